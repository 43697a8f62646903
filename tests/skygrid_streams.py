"""The (key, id) random streams of csrc/emat_gamma_pure.hpp restated on the CPU in numpy integers: Philox4x32-10 with the upper counter
words zero, block j of id l at counter (l << 32) | j, word 0 = x | y << 32 and word 1 = z | w << 32, and the conversions to_co / to_oo /
to_oc, the Box-Muller normal and the Marsaglia-Tsang gamma sampler on them.  The integer part is exact, so a uniform is the device's bit
for bit; log, sqrt and cos are the CPU's, so a normal or a gamma draw may differ from the device's in its last bits.  Vectorised over keys."""
import numpy as np

ID_TAU, ID_I_BAR, ID_ZERO_U, ID_DT, ID_HMC_U = 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFB, 0xFFFFFFFA   # include/emat_backend.h
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr, key: uint64 arrays (broadcast) -> four uint64 arrays holding the 32-bit output words."""
    ctr = np.asarray(ctr, np.uint64); key = np.asarray(key, np.uint64)
    ctr, key = np.broadcast_arrays(ctr, key)
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2 = np.zeros_like(c0); c3 = np.zeros_like(c0)
    k0, k1 = key & _M32, key >> np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0; n1 = p1 & _M32; n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1; n3 = p0 & _M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32; k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def word(key, stream_id, index):
    """64-bit word `index` (0, 1, 2, ...) of stream (key, stream_id), as site_stream_next64 hands them out."""
    block = np.uint64(index >> 1)
    w = philox4x32_10((np.uint64(stream_id) << np.uint64(32)) | block, key)
    lo, hi = (w[0], w[1]) if index % 2 == 0 else (w[2], w[3])
    return lo | (hi << np.uint64(32))


def to_co(a):
    return (a >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def to_oo(a):
    return ((a >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def to_oc(a):
    return ((a >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53


def normal(key, stream_id, first_word=0):
    u1, u2 = to_oc(word(key, stream_id, first_word)), to_co(word(key, stream_id, first_word + 1))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2)


def gamma_draw(key, stream_id, shape, rate):
    """gamma_draw of emat_gamma_pure.hpp for every key, from the start of the stream; shape and rate arrays or scalars.  A shape below 1 is
    drawn at shape + 1 and multiplied by u^(1 / shape), u the stream's next word in the open interval."""
    key = np.atleast_1d(np.asarray(key, np.uint64))
    shape = np.broadcast_to(np.asarray(shape, np.float64), key.shape); rate = np.broadcast_to(np.asarray(rate, np.float64), key.shape)
    boost = shape < 1.0
    d = np.where(boost, shape + 1.0, shape) - 1.0 / 3.0; c = 1.0 / np.sqrt(9.0 * d)
    g = d.copy(); done = np.zeros(key.shape, bool)
    at = np.zeros(key.shape, np.int64)                     # words taken so far, per key
    for _ in range(64):
        if done.all():
            break
        idx = np.flatnonzero(~done)
        x = np.empty(idx.shape); u = np.empty(idx.shape); ok = np.zeros(idx.shape, bool)
        for a in np.unique(at[idx]):                       # (keys at the same stream position share a call)
            sel = at[idx] == a
            x[sel] = normal(key[idx][sel], stream_id, int(a))
        v = 1.0 + c[idx] * x
        pos = v > 0.0
        at[idx] += 2
        for a in np.unique(at[idx][pos]):
            sel = pos & (at[idx] == a)
            u[sel] = to_oo(word(key[idx][sel], stream_id, int(a)))
        at[idx[pos]] += 1
        v3 = np.where(pos, v, 1.0) ** 3
        x2 = x * x
        with np.errstate(invalid="ignore"):
            ok[pos] = ((u < 1.0 - 0.0331 * (x2 * x2)) | (np.log(np.where(pos, u, 0.5)) < 0.5 * x2 + d[idx] * (1.0 - v3 + np.log(v3))))[pos]
        g[idx[ok]] = (d[idx] * v3)[ok]
        done[idx[ok]] = True
    if boost.any():
        idx = np.flatnonzero(boost); u = np.empty(idx.shape)
        for a in np.unique(at[idx]):
            sel = at[idx] == a
            u[sel] = to_oo(word(key[idx][sel], stream_id, int(a)))
        g[idx] *= np.exp(np.log(u) / shape[idx])
    return g / rate

"""The rules of aligned-FASTA input restated in NumPy / plain Python (include/emat_backend.h: emat_align_*; include/emat_host.h:
emat_seq_id_date_range, emat_fasta_*), written from the rules and sharing nothing with the library:

  code      a character's 4-bit set of bases, A 1, C 2, G 4, T 8; case-insensitive; U = T; N - ? . = 15; anything else 0 = no sequence letter
  valid     a row is valid when every character is a sequence letter; otherwise its first bad site and the byte there are reported
  counts    per site, over the VALID rows (dated or not), how often each of A C G T stands there unambiguously
  consensus per site the state with the largest count, ties to A, then C, then G, then T; a site never seen unambiguously is A
  tips      the rows that are valid and dated, in input order; against the reference sequence (given, or the consensus) a tip has
            deltas (site, to) at its unambiguous sites that differ, missing intervals [start, end) = the maximal runs of ambiguous codes,
            and a count of ambiguous codes other than N
  dates     a suffix of the id after '|' or '-': YYYY-MM-DD/YYYY-MM-DD, YYYY-MM-DD, YYYY-MM, YYYY, tried in that order; days since 2020-01-01;
            a month or year gives [its first day, the first day of the next]; an impossible month or day is no date
  framing   lines end at '\\n'; empty lines and lines starting with ';' are skipped; '>' starts a record whose id is the rest of the line
            stripped at both ends; white space inside sequence lines is skipped; data before the first '>' is a record named ''."""
import datetime

import numpy as np

_SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 1 | 4, "Y": 2 | 8, "S": 4 | 2, "W": 1 | 8, "K": 4 | 8, "M": 1 | 2,
         "B": 2 | 4 | 8, "D": 1 | 4 | 8, "H": 1 | 2 | 8, "V": 1 | 2 | 4, "N": 15, "-": 15, "?": 15, ".": 15}
CODE = np.zeros(256, np.uint8)
for _ch, _v in _SETS.items():
    CODE[ord(_ch)] = _v
    CODE[ord(_ch.lower())] = _v
LETTERS = "".join(sorted(set("".join(_SETS)) | set("".join(_SETS).lower())))   # every sequence letter, both cases
_STATE_OF_CODE = {1: 0, 2: 1, 4: 2, 8: 3}
_WHITE = b" \t\n\v\f\r"
_EPOCH = datetime.date(2020, 1, 1)


def is_ambiguous(codes):
    codes = np.asarray(codes, np.int64)
    return (codes & (codes - 1)) != 0


def as_rows(rows, L=None):
    """A list of equally long str / bytes, or a 2-d uint8 array, as a [rows, L] uint8 array."""
    if isinstance(rows, np.ndarray):
        return np.ascontiguousarray(rows, np.uint8)
    rows = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]
    if not rows:
        return np.zeros((0, L or 0), np.uint8)
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), len(rows[0])).copy()


def state_counts(codes, valid):
    L = codes.shape[1]
    counts = np.zeros((L, 4), np.int32)
    for code, a in _STATE_OF_CODE.items():
        counts[:, a] = np.count_nonzero(codes[valid] == code, axis=0)
    return counts


def consensus(counts):
    return np.argmax(counts, axis=1).astype(np.uint8)   # (argmax takes the first maximum: A, C, G, T; all zero -> A)


def tip_desc(code_row, ref):
    """((sites, to), (starts, ends), ambiguous codes other than N) of one tip against `ref`."""
    if len(code_row) != len(ref):
        raise ValueError("the row has %d sites and the reference sequence %d" % (len(code_row), len(ref)))
    amb = is_ambiguous(code_row)
    state = np.zeros(len(code_row), np.int64)
    for code, a in _STATE_OF_CODE.items():
        state[code_row == code] = a
    sites = np.flatnonzero(~amb & (state != ref))
    edge = np.diff(np.concatenate(([0], amb.astype(np.int8), [0])))
    return (sites.astype(np.int32), state[sites].astype(np.uint8)), (np.flatnonzero(edge == 1).astype(np.int32), np.flatnonzero(edge == -1).astype(np.int32)), \
        int(np.count_nonzero(amb & (code_row != 15)))


def finish(rows, ref=None, dated=None):
    """Everything emat_align_finish / emat_align_get return, as a dict of arrays named as in emat_align_arrays."""
    rows = as_rows(rows)
    R, L = rows.shape
    codes = CODE[rows]
    bad = codes == 0
    valid = ~bad.any(axis=1)
    bad_site = np.where(valid, -1, bad.argmax(axis=1)).astype(np.int32)
    bad_byte = np.where(valid, 0, rows[np.arange(R), np.maximum(bad_site, 0)] if L else 0).astype(np.uint8)
    counts = state_counts(codes, valid)
    ref = consensus(counts) if ref is None else np.asarray(ref, np.uint8)
    dated = np.ones(R, bool) if dated is None else np.asarray(dated).astype(bool)
    status = np.where(~valid, -2, np.where(~dated, -1, 0)).astype(np.int32)
    loss = np.zeros(R, np.int32)
    d_off, m_off, d_site, d_to, m_start, m_end = [0], [0], [], [], [], []
    for r in range(R):
        if status[r] < 0:
            continue
        status[r] = len(d_off) - 1
        (s, to), (a, b), n = tip_desc(codes[r], ref)
        d_site.append(s); d_to.append(to); m_start.append(a); m_end.append(b); loss[r] = n
        d_off.append(d_off[-1] + len(s)); m_off.append(m_off[-1] + len(a))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)   # noqa: E731
    return dict(delta_offset=np.array(d_off, np.int32), delta_site=cat(d_site, np.int32), delta_to=cat(d_to, np.uint8),
                miss_offset=np.array(m_off, np.int32), miss_start=cat(m_start, np.int32), miss_end=cat(m_end, np.int32),
                ref_sequence=ref, counts=counts, row_status=status, row_bad_site=bad_site, row_bad_byte=bad_byte, row_precision_loss=loss)


# ---- dates ------------------------------------------------------------------------------------------------------------------

def days(y, m, d):
    return float((datetime.date(y, m, d) - _EPOCH).days)


def _date(s):
    if not (len(s) == 10 and s[:4].isdigit() and s[4] == "-" and s[5:7].isdigit() and s[7] == "-" and s[8:].isdigit() and s.isascii()):
        return None
    return (int(s[:4]), int(s[5:7]), int(s[8:]))


def date_range(seq_id):
    """(t_min, t_max) or None."""
    def suffix(n):
        return seq_id[-n:] if len(seq_id) > n and seq_id[-n - 1] in "|-" else None
    try:
        s = suffix(21)
        if s and s[10] == "/" and _date(s[:10]) and _date(s[11:]):
            return days(*_date(s[:10])), days(*_date(s[11:]))
        s = suffix(10)
        if s and _date(s):
            return days(*_date(s)), days(*_date(s))
        s = suffix(7)
        if s and s.isascii() and s[:4].isdigit() and s[4] == "-" and s[5:].isdigit():
            y, m = int(s[:4]), int(s[5:])
            return days(y, m, 1), days(y + (m == 12), m % 12 + 1, 1)
        s = suffix(4)
        if s and s.isascii() and s.isdigit():
            return days(int(s), 1, 1), days(int(s) + 1, 1, 1)
    except ValueError:   # a month or a day that does not exist
        return None
    return None


# ---- framing ----------------------------------------------------------------------------------------------------------------

def frame(text):
    """[(id, sequence characters)] of a FASTA text given as bytes."""
    out, cur = [], None
    for line in text.split(b"\n"):
        if not line or line[:1] == b";":
            continue
        if line[:1] == b">":
            cur = [line[1:].strip(_WHITE).decode("latin-1"), bytearray()]
            out.append(cur)
            continue
        if cur is None:
            cur = ["", bytearray()]
            out.append(cur)
        cur[1] += bytes(c for c in line if c not in _WHITE)
    return [(name, bytes(seq)) for name, seq in out]


def render_fasta(names, rows, width=70, line_end="\n"):
    """FASTA text (bytes) of rows given as bytes / str, sequence lines of `width` characters."""
    parts = []
    for name, row in zip(names, rows):
        row = row.decode("latin-1") if isinstance(row, (bytes, bytearray)) else row
        parts.append(">" + name + line_end + "".join(row[i:i + width] + line_end for i in range(0, len(row), width)))
    return "".join(parts).encode("latin-1")

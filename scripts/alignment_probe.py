"""What aligned-FASTA input costs at C4's size (100 000 rows of 29 903 sites, 3 GB of characters), as one JSON line into
profiles/alignment_probe_latest.json.  Rows are generated chunk by chunk from a random reference sequence with C4's density: about 30
substitutions a row and 2 gaps of 270 sites in the mean (delphy_amd/scenarios.py); two chunks of 1 024 rows are made and used in turn.
In ONE process, 30 repeats each, median and p10-p90 in milliseconds of wall time, the device idle before and after every measurement:
  copy     the chunks from page-locked memory to the device and nothing else (torch): the floor of any load
  push     emat_align_push_rows of the same chunks from the handle's own page-locked buffers: that copy, k_al_code and k_al_count
  kernels  push - copy, repeat by repeat (both are serial on one stream); beside it the bytes the two kernels move -- the characters read, the
           packed codes written and read again -- per second, and that as a fraction of the 8 TB/s of HBM
  finish   emat_align_finish over all rows (consensus, counts per tip, scan, the records) and emat_align_get of everything
  load     emat_fasta_load_memory of the same rows as FASTA text (60 characters a line, dated ids): framing on one host thread into the two
           buffers, the pushes, finish; EMAT_PROBE_LOAD_REPEATS of them (default 30)
Usage: python scripts/alignment_probe.py   (EMAT_PROBE_ROWS, EMAT_PROBE_SITES, EMAT_PROBE_REPEATS: smaller figures for a trial run)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = int(os.environ.get("EMAT_PROBE_ROWS", 100000))
SITES = int(os.environ.get("EMAT_PROBE_SITES", 29903))
REPEATS = int(os.environ.get("EMAT_PROBE_REPEATS", 30))
LOAD_REPEATS = int(os.environ.get("EMAT_PROBE_LOAD_REPEATS", REPEATS))
CHUNK = 1024
HBM_BYTES_PER_S = 8e12


def _summary(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "repeats": len(ms)}


def make_chunk(rng, ref_chars):
    rows = np.tile(ref_chars, (CHUNK, 1))
    for r in range(CHUNK):
        sites = rng.integers(0, SITES, rng.poisson(30.0 * SITES / 29903))
        rows[r, sites] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(sites))]
        for _ in range(2):
            a = int(rng.integers(0, SITES)); rows[r, a:a + 1 + int(rng.exponential(270.0 * SITES / 29903))] = ord("N")
    return rows


def main():
    import torch
    import delphy_amd as d
    torch.cuda.init()
    rng = np.random.default_rng(20261021)
    ref_chars = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, SITES)]
    chunks = [make_chunk(rng, ref_chars) for _ in range(2)]
    pieces = [min(CHUNK, ROWS - at) for at in range(0, ROWS, CHUNK)]
    b = d.EmatBackend(SITES)
    lib = d.load_library()
    bufs = []
    for k in range(2):   # the handle's two page-locked row buffers, filled once
        p = C.POINTER(C.c_uint8)()
        b._ck(lib.emat_align_row_buffer(b.handle, k, CHUNK * SITES, C.byref(p)), "emat_align_row_buffer")
        view = np.ctypeslib.as_array(p, shape=(CHUNK, SITES))
        view[:] = chunks[k]
        bufs.append((p, view))
    pinned = [torch.from_numpy(c).pin_memory() for c in chunks]
    on_device = torch.empty((CHUNK, SITES), dtype=torch.uint8, device="cuda")
    copy, push, finish = [], [], []
    report = None
    for rep in range(REPEATS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, n in enumerate(pieces):
            on_device[:n].copy_(pinned[k & 1][:n], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        b.align_begin(ROWS)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for k, n in enumerate(pieces):
            b._ck(lib.emat_align_push_rows(b.handle, n, bufs[k & 1][0], SITES), "emat_align_push_rows")
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        al = b.align_finish()
        t4 = time.perf_counter()
        report = al.report
        if rep:   # the first repeat pays the allocations
            copy.append((t1 - t0) * 1e3); push.append((t3 - t2) * 1e3); finish.append((t4 - t3) * 1e3)
    kernels = [p - c for p, c in zip(push, copy)]
    chars = ROWS * SITES
    kernel_bytes = chars + 2 * ROWS * ((SITES + 1) // 2)
    line = {"rows": ROWS, "sites": SITES, "chunk_rows": CHUNK, "characters": chars, "build_id": d.source_build_id(), "date": time.strftime("%Y-%m-%d"),
            "copy": _summary(copy), "push": _summary(push), "kernels_push_minus_copy": _summary(kernels), "finish_and_get": _summary(finish), "finish_report": report,
            "copy_bytes_per_s": chars / (np.median(copy) * 1e-3), "kernel_bytes": kernel_bytes}
    km = float(np.median(kernels))
    if km > 0:
        line["kernel_bytes_per_s"] = kernel_bytes / (km * 1e-3)
        line["kernel_fraction_of_8TBps"] = line["kernel_bytes_per_s"] / HBM_BYTES_PER_S
    b.align_begin(0)
    # the whole load, from FASTA text
    if LOAD_REPEATS > 0:
        parts = []
        for r in range(ROWS):
            row = chunks[(r // CHUNK) & 1][r % CHUNK].tobytes()
            parts.append(b">hCoV-19/probe/%d/2021|EPI_ISL_%d|2021-%02d-%02d\n" % (r, r, 1 + r % 12, 1 + r % 28))
            parts.append(b"\n".join(row[i:i + 60] for i in range(0, SITES, 60)) + b"\n")
        text = b"".join(parts); del parts
        load = []
        for rep in range(LOAD_REPEATS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tips = b.load_fasta(text, chunk_rows=CHUNK)
            t1 = time.perf_counter()
            if rep:
                load.append((t1 - t0) * 1e3)
        line["load"] = _summary(load); line["load_text_bytes"] = len(text); line["load_report"] = tips.report
        line["load_over_copy"] = float(np.median(load) / np.median(copy))
    b.close()
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "alignment_probe_latest.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

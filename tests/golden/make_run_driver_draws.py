"""Generator of tests/golden/run_driver_draws.json: what the run driver draws on the tree of tests/test_run_draws_golden.py (stencils, pick,
part-size refinement, part seeds) at the recorded cycles, with the library as it is when this is run.  Recorded with the library BEFORE a
change of the driver and compared against the one after it.
Usage: python tests/golden/make_run_driver_draws.py      (EMAT_LIB_PATH=<library> to record with another build)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_run_draws_golden as T  # noqa: E402

if __name__ == "__main__":
    out = {"source": "emat_run_* of the library's host driver on the integer-built tree of tests/test_run_draws_golden.py, written by tests/golden/make_run_driver_draws.py",
           "settings": {"num_tips": T.NUM_TIPS, "seed": T.SEED, "num_parts": T.NUM_PARTS, "cycles": T.CYCLES}, "tree_checksum": T.tree_checksum(T.build_tree())}
    for limit in T.LIMITS:
        out["max_part_nodes=%d" % limit] = T.record(limit)
    json.dump(out, open(T.GOLDEN, "w"), separators=(",", ":"), sort_keys=True)   # (compact: some 170 parts a cycle with the limit on)
    print({k: {c: v[c]["partition_stats"] for c in v} for k, v in out.items() if k.startswith("max_part")})

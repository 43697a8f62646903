"""Generator of tests/golden/tree_preconditions.json: status code and last_error of every emat_tree_* entry point in every state of the
resident tree (tests/test_tree_stages_gpu.py: record_preconditions), with the library as it is when this is run.  Recorded with the
library BEFORE a change of the resident tree's host layer and compared against the one after it.  Needs the GPU.
Usage: python tests/golden/make_tree_preconditions.py [out.json]      (EMAT_LIB_PATH=<library> to record with another build)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import delphy_amd as d  # noqa: E402
import test_tree_stages_gpu as T  # noqa: E402

if __name__ == "__main__":
    out = {"source": "emat_tree_* of the library on the %d-tip tree of tests/test_tree_stages_gpu.py, written by tests/golden/make_tree_preconditions.py" % T.TIPS,
           "emat_build_id": d.library_build_id(), "table": T.record_preconditions()}
    json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN, "w"), indent=1, sort_keys=True)
    print({state: sum(1 for st, _ in calls.values() if st != 0) for state, calls in out["table"].items()}, "refusals per state")

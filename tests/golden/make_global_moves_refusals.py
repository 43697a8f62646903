"""Generator of tests/golden/global_moves_refusals.json: status code and last-error text of the global moves' entry points, with the library as
it is when this is run.  Recorded with the library BEFORE a change of the global moves' host layers and compared against the one after it.
  "host_only": the backend's entry points on a handle without a device and the run driver's calls on a run without a backend
               (tests/test_global_moves_refusals.py: record_refusals).  No GPU.
  "tree":      the resident tree's refusals by tree state and grid (tests/test_global_moves_frame_gpu.py: record_tree_refusals).  Needs the GPU.
  "parts_host_only": "host_only" for the two groups that read the parts' substitution statistics, the substitution-model moves and the APOBEC model's
               (tests/test_parts_moves_refusals.py: record_refusals).  No GPU.
  "parts":     the refusals of the three calls on the parts' statistics by the handle's state (tests/test_parts_moves_frame_gpu.py: record_parts_refusals).  Needs the GPU.
A part that is not recorded is kept as the file has it.
Usage: python tests/golden/make_global_moves_refusals.py host_only|tree|parts_host_only|parts [out.json]      (EMAT_LIB_PATH=<library> to record with another build)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import delphy_amd as d  # noqa: E402

if __name__ == "__main__":
    part = sys.argv[1]
    if part == "host_only":
        import test_global_moves_refusals as T
        table = T.record_refusals()
    elif part == "tree":
        import test_global_moves_frame_gpu as T
        table = T.record_tree_refusals()
    elif part == "parts_host_only":
        import test_parts_moves_refusals as T
        table, model_changed = T.record_refusals()
        assert model_changed == [], model_changed
    else:
        assert part == "parts", part
        import test_parts_moves_frame_gpu as T
        table = T.record_parts_refusals()
    path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    out = json.load(open(path)) if os.path.exists(path) else {}
    out["source"] = "the library's global-move entry points, written by tests/golden/make_global_moves_refusals.py"
    out[part] = table
    out.setdefault("emat_build_id", {})[part] = d.library_build_id()
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print(part, len(table), "rows")

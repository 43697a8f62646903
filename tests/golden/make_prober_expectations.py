"""Generator of tests/golden/prober_expectations.json (run where the reference tree exists).

Reads the reference's unit tests of its tree probers and turns them into DATA: inputs, expected numbers, and the tolerance
the reference's own matcher states.  Covered:

  * tests/staircase_tests.cpp                  add_boxcar, add_trapezoid and their four overlap cases: the calls in order and every
                                               at_cell expectation (closed-form right-hand sides evaluated);
  * tests/tree_prober_tests.cpp                trivial, simple, skip_one: the family, the boxcars, cells_to_skip, p_initial, and every
                                               expectation on p(i).at(x) -- equalities, DoubleNear, and the two order relations;
  * tests/ancestral_tree_prober_tests.cpp      the fixture tree, and empty, trivial, typical (both population models), skipped_ancestor;
  * tests/site_states_tree_prober_tests.cpp    trivial, typical_const_pop_model, typical_exp_pop_model with their fixture tree.

Where the reference states an expectation as code (a loop over cells that bounds every value and sums them), the case names
the rule ("each_ge", "each_eq", "cells": bounds and sum) and records the numbers the code uses, exactly as written there
(the ancestral test's 1e6 bounds included).  States are A C G T = 0 1 2 3; a mutation is [from, site, to, t].
Usage: python tests/golden/make_prober_expectations.py [/root/reference]"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_expectations import REF, cxx_eval, split_args, statements, strip_comments, test_blocks  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prober_expectations.json")
STATE = {"rA": 0, "rC": 1, "rG": 2, "rT": 3}
FLT_MAX = 3.4028234663852886e38


def _env_of(stmts, env=None):
    """Numeric `auto x = <expr>` definitions, in order (later ones may use earlier ones)."""
    env = dict(env or {})
    for st in stmts:
        m = re.match(r"(?:const )?(?:auto|double|int) (\w+) = (.*)$", st)
        if not m:
            continue
        expr = re.sub(r"static_cast<int>\((.*)\)$", r"int(\1)", m.group(2))
        try:
            v = eval(re.sub(r"std::", "", expr), {"__builtins__": {}}, {"round": round, "int": int, **env})
        except Exception:
            continue
        if isinstance(v, (int, float)):
            env[m.group(1)] = v
    return env


def staircase_cases():
    wanted = ("add_boxcar_overlaps_domain", "add_boxcar_doesnt_overlap_domain", "add_boxcar", "add_trapezoid_overlaps_domain", "add_trapezoid_doesnt_overlaps_domain", "add_trapezoid")
    out = []
    for name, line, body in test_blocks(os.path.join(REF, "tests", "staircase_tests.cpp")):
        if name not in wanted:
            continue
        steps = []
        for st in statements(body):
            m = re.match(r"auto staircase = Staircase\{(.*)\}$", st)
            if m:
                a = split_args(m.group(1)); steps.append({"op": "new", "x_start": cxx_eval(a[0], {}), "x_end": cxx_eval(a[1], {}), "num_cells": int(a[2])}); continue
            m = re.match(r"(add_boxcar|add_trapezoid)\(staircase, (.*)\)$", st)
            if m:
                steps.append({"op": m.group(1), "args": [cxx_eval(a, {}) for a in split_args(m.group(2))]}); continue
            m = re.match(r"EXPECT_EQ\(staircase\.at_cell\((\d+)\), (.*)\)$", st)
            if m:
                steps.append({"op": "expect", "cell": int(m.group(1)), "value": cxx_eval(m.group(2), {}), "tol": 0.0}); continue
            m = re.match(r"EXPECT_THAT\(staircase\.at_cell\((\d+)\), testing::DoubleNear\((.*), ([0-9.e+-]+)\)\)$", st)
            if m:
                steps.append({"op": "expect", "cell": int(m.group(1)), "value": cxx_eval(m.group(2), {}), "tol": float(m.group(3))}); continue
            raise SystemExit("staircase_tests.cpp %s: not understood: %s" % (name, st))
        out.append({"test": name, "line": line, "steps": steps})
    assert len(out) == len(wanted)
    return out


def _matcher(text, env, members):
    m = re.match(r"Eq\((.*)\)$", text)
    if m:
        return {"matcher": "eq", "value": cxx_eval(m.group(1), env)}
    m = re.match(r"DoubleNear\((.*), ([0-9.e+-]+)\)$", text)
    if m:
        return {"matcher": "near", "value": cxx_eval(m.group(1), env), "tol": float(m.group(2))}
    m = re.match(r"Gt\((\w+)\.at\((.*)\)\)$", text)
    if m:
        return {"matcher": "gt_other", "other_member": members[m.group(1)], "other_x": cxx_eval(m.group(2), env)}
    m = re.match(r"Gt\((.*)\)$", text)
    if m:
        return {"matcher": "gt", "value": cxx_eval(m.group(1), env)}
    raise SystemExit("matcher not understood: " + text)


def tree_prober_cases():
    out = []
    for name, line, body in test_blocks(os.path.join(REF, "tests", "tree_prober_tests.cpp")):
        if name not in ("trivial", "simple", "skip_one"):
            continue
        stmts = statements(body)
        env = _env_of(stmts)
        case = {"test": name, "line": line, "pop": {"kind": "const", "pop": env["pop"]}, "num_cats": env["num_cats"], "t_start": env["t_start"], "t_end": env["t_end"],
                "num_cells": env["num_cells"], "cells_to_skip": env["cells_to_skip"], "p_initial": None, "boxcars": [], "expect": []}
        counts, members = {}, {}
        for st in stmts:
            m = re.match(r"auto& (\w+) = branch_counts_by_cat\[(\d+)\]$", st)
            if m:
                counts[m.group(1)] = int(m.group(2)); continue
            m = re.match(r"auto& (\w+) = tree_prober\.p\((\d+)\)$", st)
            if m:
                members[m.group(1)] = int(m.group(2)); continue
            m = re.match(r"auto p_initial = std::vector\{(.*)\}$", st)
            if m:
                case["p_initial"] = [cxx_eval(a, env) for a in split_args(m.group(1))]; continue
            m = re.match(r"add_boxcar\((\w+), (.*)\)$", st)
            if m:
                case["boxcars"].append({"member": counts[m.group(1)], "args": [cxx_eval(a, env) for a in split_args(m.group(2))]}); continue
            m = re.match(r"EXPECT_THAT\(tree_prober\.p\((\d+)\)\.at\((.*?)\), (.*)\)$", st) or re.match(r"EXPECT_THAT\((p_\d+)\.at\((.*?)\), (.*)\)$", st)
            if m:
                member = int(m.group(1)) if m.group(1).isdigit() else members[m.group(1)]
                case["expect"].append({"member": member, "x": cxx_eval(m.group(2), env), **_matcher(m.group(3), env, members)}); continue
            m = re.match(r"EXPECT_THAT\(tree_prober\.t_start\(\), testing::DoubleNear\((.*), ([0-9.e+-]+)\)\)$", st)
            if m:
                case["expect_t_start"] = {"value": cxx_eval(m.group(1), env), "tol": float(m.group(2))}; continue
            m = re.match(r"EXPECT_EQ\(tree_prober\.(t_start|t_end)\(\), (\w+)\)$", st)
            if m:
                case["expect_" + m.group(1)] = {"value": env[m.group(2)], "tol": 0.0}; continue
        assert case["expect"], name
        out.append(case)
    assert len(out) == 3
    return out


def _fixture_tree(text, index_pattern):
    """The tree a fixture builds with `tree.at(x).<field> = ...` statements: nodes by index, the reference sequence, the root."""
    idx = {m.group(1): int(m.group(2)) for m in re.finditer(index_pattern, text)}
    n = int(re.search(r"Phylo_tree(?: tree)?\{(\d+)\}", text).group(1))
    ref = [STATE[s.strip()] for s in re.search(r"Real_sequence(?: ref_sequence)?\{([^}]*)\}", text).group(1).split(",")]
    nodes = [{"parent": -1, "children": [], "t": 0.0, "t_min": -FLT_MAX, "t_max": FLT_MAX, "mutations": []} for _ in range(n)]
    root = None
    for piece in strip_comments(text).split(";"):     # (the statements sit inside a constructor or function body)
        found = re.search(r"(tree\.(?:root|at\(\w+\)\.\w+) = .*)$", " ".join(piece.split()))
        if not found:
            continue
        st = found.group(1)
        m = re.match(r"tree\.root = (\w+)$", st)
        if m:
            root = idx.get(m.group(1), int(m.group(1)) if m.group(1).isdigit() else None); continue
        m = re.match(r"tree\.at\((\w+)\)\.parent = (\w+)$", st)
        if m:
            nodes[idx[m.group(1)]]["parent"] = -1 if m.group(2) == "k_no_node" else idx[m.group(2)]; continue
        m = re.match(r"tree\.at\((\w+)\)\.children = \{(.*)\}$", st)
        if m:
            nodes[idx[m.group(1)]]["children"] = [idx[c.strip()] for c in m.group(2).split(",") if c.strip()]; continue
        m = re.match(r"tree\.at\((\w+)\)\.t = tree\.at\(\w+\)\.t_min = tree\.at\(\w+\)\.t_max = (.*)$", st)
        if m:
            v = cxx_eval(m.group(2), {}); nodes[idx[m.group(1)]].update(t=v, t_min=v, t_max=v); continue
        m = re.match(r"tree\.at\((\w+)\)\.t = (.*)$", st)
        if m:
            nodes[idx[m.group(1)]]["t"] = cxx_eval(m.group(2), {}); continue
        m = re.match(r"tree\.at\((\w+)\)\.mutations = \{(.*)\}$", st)
        if m:
            nodes[idx[m.group(1)]]["mutations"] = [[STATE[a.strip()], int(s), STATE[b.strip()], float(t)] for a, s, b, t in re.findall(r"Mutation\{(\w+), (\d+), (\w+), ([0-9.e+-]+)\}", m.group(2))]
    return {"names": {k: v for k, v in idx.items()}, "root": root, "ref_sequence": ref, "nodes": nodes}


def _grid(env):
    return {"t_start": env["t_start"], "t_end": env["t_end"], "num_t_cells": int(env.get("num_t_cells", env.get("num_cells")))}


def ancestral_cases():
    src = open(os.path.join(REF, "tests", "ancestral_tree_prober_tests.cpp")).read()
    fixture_text = src[src.index("class Ancestral_tree_prober_test"): src.index("TEST_F(")]
    tree = _fixture_tree(fixture_text, r"static constexpr Node_index (\w+) = (\d+);")
    fenv = {m.group(1): float(m.group(2)) for m in re.finditer(r"double (\w+)\{([0-9.e+-]+)\};", fixture_text)}
    pops = {"Constant": {"kind": "const", "pop": fenv["const_pop"]}, "Exponential": {"kind": "exp", "t0": 0.0, "n0": fenv["exp_pop_n0"], "g": fenv["exp_pop_g"], "min_pop": 0.0}}
    m = re.search(r"Exp_pop_model exp_pop_model\{(.*?)\}", fixture_text)
    a = split_args(m.group(1)); pops["Exponential"].update(t0=cxx_eval(a[0], fenv), min_pop=cxx_eval(a[3], fenv))
    names = tree["names"]
    cases = []
    for name, line, body in test_blocks(os.path.join(REF, "tests", "ancestral_tree_prober_tests.cpp")):
        if name not in ("empty", "trivial", "typical", "skipped_ancestor"):
            continue
        stmts = statements(body.replace("{ SCOPED_TRACE", "; SCOPED_TRACE")) if name != "typical" else statements(re.search(r"SCOPED_TRACE\(pop_model_name\);(.*?)// Check|SCOPED_TRACE\(pop_model_name\);(.*)", body, flags=re.S).group(0))
        env = _env_of(stmts)
        marked = re.search(r"marked_ancestors = std::vector(?:<Node_index>)?\{([^}]*)\}", body).group(1)
        case = {"test": name, "line": line, **_grid(env), "marked": [-1 if v.strip() == "k_no_node" else names[v.strip()] for v in marked.split(",") if v.strip()]}
        if name == "empty":
            case.update(pops=["Constant"], num_members=int(re.search(r"num_members\(\), testing::Eq\((\d+)\)", body).group(1)),
                        each_ge=[{"member": 0, "value": cxx_eval(re.search(r"Each\(testing::Ge\((.*?)\)\)", body).group(1), {})}])
        elif name == "trivial":
            case.update(pops=["Constant"], at=[{"member": int(i), "x": env["t_start"], "value": float(v), "tol": float(t)}
                                              for i, v, t in re.findall(r"results\[(\d+)\]\.at\(t_start\), testing::DoubleNear\(([0-9.]+), ([0-9.e+-]+)\)", body)])
        elif name == "typical":
            case.update(pops=["Constant", "Exponential"], cells={"members": "marked", "each_ge": cxx_eval(re.search(r"testing::Ge\((.*?)\)", body).group(1), {}),
                                                                  "each_le": cxx_eval(re.search(r"testing::Le\((.*?)\)", body).group(1), {}),
                                                                  "sum_near": [float(x) for x in re.search(r"EXPECT_THAT\(tot_p, testing::DoubleNear\(([0-9.]+), ([0-9.e+-]+)\)\)", body).groups()]})
        else:
            case.update(pops=["Constant"], each_eq=[{"member": int(i), "value": float(v)} for i, v in re.findall(r"results\[(\d+)\], testing::Each\(testing::Eq\(([0-9.]+)\)\)", body)])
        cases.append(case)
    assert len(cases) == 4
    return {"tree": tree, "pops": pops, "cases": cases}


def site_states_cases():
    path = os.path.join(REF, "tests", "site_states_tree_prober_tests.cpp")
    src = open(path).read()
    body_text = src[src.index("static auto site_states_tree_prober_test_body"): src.index("TEST(Site_states_tree_prober_test, typical_const_pop_model)")]
    tree = _fixture_tree(body_text, r"const auto (\w+) = Node_index\{(\d+)\};")
    env = _env_of(statements(strip_comments(body_text[body_text.index("{") + 1:])))
    cells = {"members": "all", "each_ge": cxx_eval(re.search(r"testing::Ge\((.*?)\)", body_text).group(1), {}), "each_le": cxx_eval(re.search(r"testing::Le\((.*?)\)", body_text).group(1), {}),
             "sum_near": [float(x) for x in re.search(r"EXPECT_THAT\(tot_p, testing::DoubleNear\(([0-9.]+), ([0-9.e+-]+)\)\)", body_text).groups()]}
    site = int(re.search(r"auto site = Site_index\{(\d+)\}", body_text).group(1))
    cases = []
    for name, line, body in test_blocks(path):
        if name == "trivial":
            tenv = _env_of(statements(body))
            t = _fixture_tree(body, r"$^")
            t["root"] = int(re.search(r"tree\.root = (\d+)", body).group(1))
            cases.append({"test": name, "line": line, "tree": t, "pop": {"kind": "const", "pop": tenv["pop"]}, "site": int(re.search(r"auto site = Site_index\{(\d+)\}", body).group(1)), **_grid(tenv),
                          "at": [{"member": STATE[s], "x": tenv["t_start"], "value": float(v), "tol": float(tol)}
                                 for s, v, tol in re.findall(r"results\[index_of\((\w+)\)\]\.at\(t_start\), testing::DoubleNear\(([0-9.]+), ([0-9.e+-]+)\)", body)]})
        elif name.startswith("typical_"):
            m = re.search(r"test_body\((Const_pop_model|Exp_pop_model)\{(.*?)\}\)", body)
            v = [cxx_eval(a, {}) for a in split_args(m.group(2))]
            pop = {"kind": "const", "pop": v[0]} if m.group(1) == "Const_pop_model" else {"kind": "exp", "t0": v[0], "n0": v[1], "g": v[2], "min_pop": v[3]}
            cases.append({"test": name, "line": line, "tree": tree, "pop": pop, "site": site, **_grid(env), "cells": cells})
    assert len(cases) == 3
    return cases


if __name__ == "__main__":
    out = {"source": "expectations of the reference's tests/staircase_tests.cpp, tree_prober_tests.cpp, ancestral_tree_prober_tests.cpp, site_states_tree_prober_tests.cpp, extracted by tests/golden/make_prober_expectations.py",
           "states": "A C G T = 0 1 2 3; a mutation is [from, site, to, t]; t_min / t_max of -+3.4e38 are the reference's -+FLT_MAX",
           "staircase": staircase_cases(), "tree_prober": tree_prober_cases(), "ancestral_tree_prober": ancestral_cases(), "site_states_tree_prober": site_states_cases()}
    json.dump(out, open(OUT, "w"), indent=0, sort_keys=True)
    print("staircase %d | tree_prober %d | ancestral %d | site_states %d" % (len(out["staircase"]), len(out["tree_prober"]), len(out["ancestral_tree_prober"]["cases"]), len(out["site_states_tree_prober"])))

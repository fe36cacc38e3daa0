"""The dependency lists of cvxpnpl_amd/build.py: for each of the twelve libraries the list that decides whether it is rebuilt is exactly the
sources of its compile command and every file they reach through quoted includes.  A header missing from a list is an edit that does
not rebuild its library; one too many is a rebuild for nothing.  No GPU needed, nothing is compiled."""
import os
import re

LIBRARIES = [("DEPS", "compile_cmd"), ("GRAD_DEPS", "grad_compile_cmd"), ("RANSAC_DEPS", "ransac_compile_cmd"),
             ("RANSAC_PNPL_DEPS", "ransac_pnpl_compile_cmd"), ("REFINE_DEPS", "refine_compile_cmd"),
             ("REFINE_GRAD_DEPS", "refine_grad_compile_cmd"), ("REFINE_ROBUST_DEPS", "refine_robust_compile_cmd"),
             ("REFINE_ROBUST_GRAD_DEPS", "refine_robust_grad_compile_cmd"), ("RANSAC_ADAPTIVE_DEPS", "ransac_adaptive_compile_cmd"),
             ("RANSAC_GUIDED_DEPS", "ransac_guided_compile_cmd"), ("RANSAC_PNPL_ADAPTIVE_DEPS", "ransac_pnpl_adaptive_compile_cmd"),
             ("REFINE_ROBUST_AUTO_DEPS", "refine_robust_auto_compile_cmd")]


def include_closure(sources):
    """the sources and every file they include by #include "...", transitively; a quoted include is looked up beside the including file"""
    seen, todo = set(), [os.path.realpath(s) for s in sources]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), flags=re.M):
                todo.append(os.path.realpath(os.path.join(os.path.dirname(path), name)))
    return seen


def test_dependency_lists_are_the_include_closures_of_the_sources():
    from cvxpnpl_amd import build

    assert sorted(n for n in dir(build) if n.endswith("compile_cmd")) == sorted(c for _, c in LIBRARIES)
    assert sorted(n for n in dir(build) if n == "DEPS" or (n.endswith("_DEPS") and n != "RANSAC_ENTRY_DEPS")) == sorted(d for d, _ in LIBRARIES)
    rel = lambda paths: sorted(os.path.relpath(p, os.path.dirname(build.HERE)) for p in paths)
    wrong = {}
    for deps, cmd in LIBRARIES:
        sources = [c for c in getattr(build, cmd)("x") if c.endswith((".hip", ".cpp"))]
        assert sources, cmd
        listed = [os.path.realpath(d) for d in getattr(build, deps)]
        assert len(listed) == len(set(listed)), (deps, "a file is listed twice")
        closure = include_closure(sources)
        if set(listed) != closure:
            wrong[deps] = {"missing from the list": rel(closure - set(listed)), "listed but not included": rel(set(listed) - closure)}
    assert not wrong, wrong

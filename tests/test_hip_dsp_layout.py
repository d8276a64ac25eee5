"""
The layout of ``qampy_amd.core.hip_dsp``, a package of one module per unit: the package exposes exactly the public names the single
module had (``tests/golden/hip_dsp_names.json``, recorded from it), and no unit borrows another unit's underscore names.
"""
import ast
import inspect
import json
import os

from qampy_amd.core import hip_dsp

HERE = os.path.dirname(os.path.abspath(__file__))
PACKAGE = os.path.dirname(os.path.abspath(hip_dsp.__file__))


def _kind(value):
    if inspect.isclass(value):
        return "class"
    return "function" if callable(value) else "constant"


def test_the_package_exposes_the_names_of_the_single_module():
    """Every public name, less the modules: a unit that forgets a re-export fails here."""
    with open(os.path.join(HERE, "golden", "hip_dsp_names.json")) as f:
        golden = json.load(f)
    names = {n: _kind(getattr(hip_dsp, n)) for n in dir(hip_dsp) if not n.startswith("_") and not inspect.ismodule(getattr(hip_dsp, n))}
    assert sorted(set(golden) - set(names)) == [], "names the package lost"
    assert sorted(set(names) - set(golden)) == [], "names the package gained"
    assert names == golden
    for n, kind in golden.items():
        if kind != "constant":
            owner = inspect.getmodule(getattr(hip_dsp, n))
            assert owner.__name__.startswith(hip_dsp.__name__ + ".") and getattr(owner, n) is getattr(hip_dsp, n), n


def _modules():
    for name in sorted(os.listdir(PACKAGE)):
        if name.endswith(".py"):
            with open(os.path.join(PACKAGE, name)) as f:
                yield name[:-3], ast.parse(f.read())


def test_no_unit_borrows_an_underscore_name_of_another():
    """Inside the package an underscore name is imported from ``_args`` alone (or is ``_args`` itself), and ``__init__`` only re-exports."""
    seen = []
    for name, tree in _modules():
        seen.append(name)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                base = hip_dsp.__name__.split(".")
                source = ".".join((base[:len(base) - node.level + 1] if node.level else []) + ([node.module] if node.module else []))
                if source != hip_dsp.__name__ and not source.startswith(hip_dsp.__name__ + "."):
                    continue                                                    # from outside the package
                unit = source[len(hip_dsp.__name__) + 1:]                       # "" for the package itself
                for a in node.names:
                    if a.name.startswith("_"):
                        assert (unit, a.name) == ("", "_args") or unit == "_args", "%s imports %s from %r" % (name, a.name, unit)
                assert unit in ("", "_args") or not unit.startswith("_"), "%s imports from %s" % (name, unit)
            if isinstance(node, ast.Import):
                assert not any(a.name.startswith(hip_dsp.__name__ + ".") for a in node.names), "%s imports a unit by its full name" % name
            if name == "__init__":
                assert not isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef, ast.Lambda)), "__init__ defines code of its own"
    assert "__init__" in seen and "_args" in seen and len(seen) == 17

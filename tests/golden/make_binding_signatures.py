"""Records tests/golden/binding_signatures.json: the restype and the argtypes the Python bindings declare on every function of
libsuper4pcs_normals.so and libsuper4pcs_icp.so.

    python tests/golden/make_binding_signatures.py          (no GPU needed; with the binding to be pinned)

record() loads both libraries through the package, declares every family and walks every symbol list of the modules
(SYMBOLS, normals.ORIENT_SYMBOLS, icp.*_SYMBOLS): name -> [restype's name or null, [the argtypes' names]].
tests/test_binding_host.py runs it again and asks for the same file, key for key, so a binding that states its signatures
another way still states these."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binding_signatures.json")
NORMALS_MODULES = ("normals", "knn", "voxel", "cluster", "plane", "shape", "features")


def _lists(module):
    return [getattr(module, a) for a in sorted(vars(module)) if a == "SYMBOLS" or a.endswith("_SYMBOLS")]


def _dump(L, names):
    out = {}
    for name in names:
        fn = getattr(L, name)
        out[name] = [None if fn.restype is None else fn.restype.__name__, [a.__name__ for a in fn.argtypes]]
    return out


def record():
    """{"normals": {name: signature}, "icp": {name: signature}} of the two libraries as the package binds them."""
    mods = [importlib.import_module("super4pcs_amd." + m) for m in NORMALS_MODULES]
    for m in mods:
        L = m.load_library()
    mods[0].load_orient()
    icp = importlib.import_module("super4pcs_amd.icp")
    return {"normals": _dump(L, [s for m in mods for names in _lists(m) for s in names]),
            "icp": _dump(icp.load_library(), [s for names in _lists(icp) for s in names])}


if __name__ == "__main__":
    from super4pcs_amd import build as B
    B.build_normals()
    B.build_icp()
    got = record()
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s -> %s" % (", ".join("%d %s" % (len(v), k) for k, v in got.items()), OUT))

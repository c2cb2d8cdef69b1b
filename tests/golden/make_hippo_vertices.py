"""The vertices of the reference's bundled hippo pair (assets/hippo1.obj, assets/hippo2.obj), so that the sampler's known answer
(tests/test_oracle.py::test_sampler_known_answer_on_reference_assets) runs without the reference.  The OBJ files print every
coordinate with six decimals, so each one is stored exactly as an integer number of millionths, delta-coded along the file
(tests/golden/hippo_vertices.npz, ~200 KB instead of 7 MB of OBJ); load() gives back what parsing the OBJ text to float32 gives.
Needs the reference's assets; run from the repo root:  python tests/golden/make_hippo_vertices.py <reference root>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "hippo_vertices.npz")


def load_obj_vertices(path):
    v = []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                v.append([float(x) for x in line.split()[1:4]])
    return np.array(v, np.float32)


def load():
    """(hippo1, hippo2) as float32 [n, 3], bit-identical to load_obj_vertices() of the two asset files."""
    with np.load(NPZ) as d:
        return tuple((np.cumsum(d[k].astype(np.int64), axis=0) / 1e6).astype(np.float32) for k in ("hippo1", "hippo2"))


def main(ref):
    out = {}
    for name in ("hippo1", "hippo2"):
        v = load_obj_vertices(os.path.join(ref, "assets", name + ".obj"))
        micro = np.round(v.astype(np.float64) * 1e6).astype(np.int64)
        assert np.array_equal((micro / 1e6).astype(np.float32), v), name
        out[name] = np.diff(micro, axis=0, prepend=0).astype(np.int32)
    np.savez_compressed(NPZ, **out)
    h1, h2 = load()
    assert np.array_equal(h1, load_obj_vertices(os.path.join(ref, "assets", "hippo1.obj")))
    assert np.array_equal(h2, load_obj_vertices(os.path.join(ref, "assets", "hippo2.obj")))
    print("wrote %s: %d + %d vertices" % (os.path.relpath(NPZ), len(h1), len(h2)))


if __name__ == "__main__":
    main(sys.argv[1])

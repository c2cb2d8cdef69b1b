"""super4pcs_amd/_binding.py and the tables the bindings state on it, without a GPU: declare with and without an error class, the
twin mark, the loader's error, the column and result helpers on numpy, every symbol list as its table's names, and every
declared signature of both libraries against tests/golden/binding_signatures.json (recorded at the commit before the tables)."""
import ctypes as C
import importlib
import json
import types

import numpy as np
import pytest

from super4pcs_amd import _binding as B
from tests.golden import make_binding_signatures as G

TABLE = {
    "f_create": [C.c_int32, C.POINTER(C.c_void_p)],
    "f_destroy": (None, [C.c_void_p]),
    "f_run" + B.TWIN: [C.c_void_p, C.c_int64],
    "f_name": (C.c_char_p, [C.c_void_p]),
}


class StubError(RuntimeError):
    REBUILD = "build.build_stub()"

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _stub(without=()):
    """An object with one attribute per function of TABLE, none declared, except the names of `without`."""
    fn = lambda: types.SimpleNamespace(restype=C.c_int, argtypes=None)
    return types.SimpleNamespace(_name="/somewhere/libstub.so", **{n: fn() for n in B.names(TABLE) if n not in without})


def test_declare_with_an_error_class_refuses_a_library_that_lacks_names_before_declaring_any():
    L = _stub(without=("f_destroy", "f_run_device"))
    with pytest.raises(StubError) as e:
        B.declare(L, TABLE, StubError)
    assert e.value.code == -7
    assert str(e.value) == "libstub.so lacks f_destroy, f_run_device: rebuild it (build.build_stub())"
    assert [n for n in ("f_create", "f_run", "f_name") if getattr(L, n).argtypes is not None or getattr(L, n).restype is not C.c_int] == []


def test_declare_without_an_error_class_skips_what_is_absent():
    L = _stub(without=("f_destroy", "f_run_device"))
    B.declare(L, TABLE)
    assert not hasattr(L, "f_destroy") and not hasattr(L, "f_run_device")
    assert L.f_create.argtypes == [C.c_int32, C.POINTER(C.c_void_p)] and L.f_create.restype is C.c_int32
    assert L.f_run.argtypes == [C.c_void_p, C.c_int64] and L.f_run.restype is C.c_int32
    assert L.f_name.argtypes == [C.c_void_p] and L.f_name.restype is C.c_char_p


def test_a_twin_entry_declares_both_forms_alike():
    L = _stub()
    B.declare(L, TABLE, StubError)
    assert B.names(TABLE) == ["f_create", "f_destroy", "f_run", "f_run_device", "f_name"]
    assert L.f_run.argtypes == L.f_run_device.argtypes == [C.c_void_p, C.c_int64]
    assert L.f_run.restype is L.f_run_device.restype is C.c_int32
    assert L.f_destroy.restype is None and L.f_destroy.argtypes == [C.c_void_p]


def test_open_library_on_a_missing_path(tmp_path):
    with pytest.raises(StubError) as e:
        B.open_library(str(tmp_path / "libnone.so"), StubError, "libnone.so")
    assert e.value.code == -7 and "libnone.so not built" in str(e.value)


def test_cols_on_numpy():
    X = np.asfortranarray(np.arange(15, dtype=np.float64).reshape(5, 3) / 7)
    dev, ptr, n, keep = B.cols(X)
    assert dev is False and n == 5 and len(ptr) == len(keep) == 3
    for k in range(3):
        assert keep[k].dtype == np.float32 and keep[k].flags["C_CONTIGUOUS"] and keep[k].shape == (5,)
        assert np.array_equal(keep[k], X[:, k].astype(np.float32)) and ptr[k] == keep[k].ctypes.data
    with pytest.raises(ValueError, match=r"^clouds are \(N, 3\)$"):
        B.cols(np.zeros((5, 2)))


def test_empty_and_sync_without_a_tensor():
    a, p = B.empty(None, (4, 3), np.int32)
    assert isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == (4, 3) and a.flags["C_CONTIGUOUS"] and p == a.ctypes.data
    assert B.sync(None) is None and not B.is_torch(a)


@pytest.fixture(scope="module")
def built():
    from super4pcs_amd import build
    build.build_normals()
    build.build_icp()


@pytest.mark.parametrize("module,table,symbols", [(m, "SIGNATURES", "SYMBOLS") for m in G.NORMALS_MODULES] + [
    ("normals", "ORIENT_SIGNATURES", "ORIENT_SYMBOLS"), ("icp", "SIGNATURES", "SYMBOLS")] + [
    ("icp", g + "_SIGNATURES", g + "_SYMBOLS") for g in ("PLANE", "ROBUST", "GICP", "SYMM", "COLOR", "REJECT", "BATCH", "INFO")] + [
    ("posegraph", "SIGNATURES", None)])
def test_a_symbol_list_is_its_table(module, table, symbols):
    mod = importlib.import_module("super4pcs_amd." + module)
    icp = importlib.import_module("super4pcs_amd.icp")
    got = getattr(mod, symbols) if symbols else icp.POSEGRAPH_SYMBOLS
    want = []
    for key in getattr(mod, table):
        want += [key[:-len("[_device]")], key[:-len("[_device]")] + "_device"] if key.endswith("[_device]") else [key]
    assert list(got) == want and len(set(got)) == len(got) and got


def test_every_list_of_icp_has_its_table_among_the_declared_ones():
    icp = importlib.import_module("super4pcs_amd.icp")
    lists = [getattr(icp, a) for a in sorted(vars(icp)) if a == "SYMBOLS" or a.endswith("_SYMBOLS")]
    assert sorted(map(list, lists)) == sorted(B.names(t) for t in icp.TABLES) and len(lists) == 10
    assert sum(len(v) for v in lists) == len({s for v in lists for s in v}) == 53


def test_signatures_equal_the_recorded_ones(built):
    got = G.record()
    with open(G.OUT) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) == ["icp", "normals"]
    for lib in want:
        assert sorted(got[lib]) == sorted(want[lib]), lib
        assert {n: got[lib][n] for n in want[lib] if got[lib][n] != want[lib][n]} == {}, lib
    assert (len(got["normals"]), len(got["icp"])) == (38, 53)


def test_a_second_path_is_a_second_library_and_the_first_stays(built, tmp_path):
    import shutil
    from super4pcs_amd import knn, normals
    first = knn.load_library()
    copy = shutil.copy(normals.LIB_PATH, str(tmp_path / "libsuper4pcs_normals.so"))
    other = knn.load_library(copy)
    assert other is not first and other is knn.load_library(copy) and first is knn.load_library() is normals.load_library()
    assert other.s4p_knn_search.argtypes == first.s4p_knn_search.argtypes and other.s4p_knn_search.argtypes is not None

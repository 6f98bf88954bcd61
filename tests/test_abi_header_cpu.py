"""CPU: the ctypes binding is read from include/muygpys_hip.h (muygpys_amd/_abi.py) -- every declared function is
bound as the header states it, a handful of signatures and every enum value are restated here independently, the
header's f32 / f64 pairs agree with each other, and the reader refuses what it does not understand."""

import ctypes as C
import os
import subprocess
import sys

import pytest

from muygpys_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

p, i, l, d, s = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_char_p

# written out by hand from the header, parameter by parameter (not the whole table: the long and the odd ones)
SPOT = {
    "mgp_posterior_f32": (i, [p, p, i, p, p, l, i, p, i, i, d, p, i, i, p, i, p, p, p, p, p]),
    "mgp_posterior_gen_f64": (i, [p, p, p, l, p, l, i, p, p, l, i, p, i, i, i, d, p, d, i, p, i, p, p, p, p, p]),
    "mgp_posterior_packed_gathered_f32": (i, [p, l, p, l, i, p, p, l, i, p, i, i, d, p, i, i, p, i, p, p, p, p, p]),
    "mgp_loocv_tree_f64": (i, [p, p, p, p, l, p, l, d, i, i, p, p, p]),
    "mgp_knn_scan_bf16x3": (i, [p, p, p, l, i, p, p, p, p, l, i, l, p, p, p, p]),
    "mgp_shear_posterior_f64": (i, [p, p, p, p, l, i, i, p, l, i, d, i, d, p, p, p, p, p]),
    "mgp_class_partition_f32": (i, [p, l, i, p, l, i, p, p, p, p, p, p, p]),
    "mgp_last_launch_geometry": (i, [p, p]),
    "mgp_jit_source_hash": (i, [s, i]),
    "mgp_version": (s, []),
    "mgp_packed_row_bytes": (l, [i, i, i]),
    "mgp_loocv_scratch_bytes": (l, []),
}
SPOT_COUNTS = {"mgp_posterior_f32": 21, "mgp_posterior_gen_f64": 26, "mgp_posterior_packed_gathered_f32": 23,
               "mgp_loocv_tree_f64": 13, "mgp_knn_scan_bf16x3": 16, "mgp_shear_posterior_f64": 18,
               "mgp_class_partition_f32": 13}

# the neighbour search is fp32 only
F32_ONLY = {"mgp_topk_rows_f32", "mgp_knn_finish_f32", "mgp_knn_scan_f32"}

ENUMS = {
    "MGP_KERNEL_RBF": 0, "MGP_KERNEL_MATERN_05": 1, "MGP_KERNEL_MATERN_15": 2, "MGP_KERNEL_MATERN_25": 3,
    "MGP_KERNEL_MATERN_INF": 4, "MGP_KERNEL_MATERN_GEN": 5,
    "MGP_METRIC_L2": 0, "MGP_METRIC_F2": 1,
    "MGP_NOISE_SCALAR": 0, "MGP_NOISE_TABLE": 1, "MGP_NOISE_BATCH": 2,
    "MGP_OK": 0, "MGP_EINVAL": -1, "MGP_EUNSUPPORTED": -2, "MGP_EHIP": -1000,
    "MGP_SHEAR_33": 0, "MGP_SHEAR_KIN23": 1, "MGP_SHEAR_KCROSS23": 2,
    "MGP_SHEAR_NOISE_HOMOSCEDASTIC": 0, "MGP_SHEAR_NOISE_33": 1,
    "MGP_CLASS_LOSS_CROSS_ENTROPY": 0, "MGP_CLASS_LOSS_MSE": 1,
}


def test_reader_covers_every_declared_function():
    from muygpys_amd import _lib

    assert set(_abi.signatures()) == set(_lib.exported_names_from_header())
    assert _abi.signatures() is _abi.signatures()  # parsed once


def test_loaded_library_is_bound_as_the_header_states():
    from muygpys_amd import _lib

    lib = _lib.load()
    for name, (restype, argtypes) in _abi.signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_spot_signatures():
    sigs = _abi.signatures()
    for name, (restype, argtypes) in SPOT.items():
        assert sigs[name] == (restype, argtypes), name
    for name, count in SPOT_COUNTS.items():
        assert len(sigs[name][1]) == count, name


def test_f32_declarations_have_identical_f64_twins():
    sigs = _abi.signatures()
    singles = set()
    for name in sigs:
        if name.endswith("_f32"):
            twin = name[:-4] + "_f64"
            if twin not in sigs:
                singles.add(name)
            else:
                assert sigs[name] == sigs[twin], name
    assert singles == F32_ONLY
    assert all(n[:-4] + "_f32" in sigs for n in sigs if n.endswith("_f64"))


@pytest.mark.parametrize("decl", ["int mgp_x(float a);", "int mgp_x(size_t n);", "int mgp_x(int (*cb)(int));",
                                  "int mgp_x(unsigned n);", "int mgp_x(struct mgp_s v);", "float mgp_x(int a);",
                                  "int mgp_x(int);", "int mgp_x();", "int mgp_x(int a"])
def test_reader_refuses_what_it_does_not_understand(decl):
    with pytest.raises(ValueError, match="mgp_x"):
        _abi.parse(decl)


def test_reader_accepts_void_and_declarations_over_several_lines():
    assert _abi.parse("int mgp_x(void);") == ({"mgp_x": (i, [])}, {})
    one = _abi.parse("int64_t mgp_x(const float* a, int64_t n, double eps, char* buf, void* stream);")
    three = _abi.parse("int64_t mgp_x(const float* a,\n    int64_t n, /* rows\n of a */ double eps,\n"
                       "    char *buf, void* stream);")
    assert one == three == ({"mgp_x": (l, [p, l, d, s, p])}, {})
    assert _abi.parse("enum mgp_e { MGP_A = 0, /* , B = 7 */ MGP_B = -3 };") == ({}, {"MGP_A": 0, "MGP_B": -3})
    with pytest.raises(ValueError, match="MGP_A"):
        _abi.parse("enum mgp_e { MGP_A, MGP_B };")


def test_bind_names_a_missing_symbol():
    class Empty:
        _name = "libnothing.so"

    with pytest.raises(AttributeError, match="mgp_"):
        _abi.bind(Empty())


def test_enum_values():
    from muygpys_amd import _lib

    assert _abi.enums() == ENUMS
    assert _lib.KERNEL_IDS == {"rbf": 0, "matern05": 1, "matern15": 2, "matern25": 3, "maternInf": 4, "matern_gen": 5}
    assert _lib.METRIC_IDS == {"l2": 0, "F2": 1}
    assert _lib.CLASS_LOSS_IDS == {"cross_entropy": 0, "mse": 1}
    assert (_lib.NOISE_SCALAR, _lib.NOISE_TABLE, _lib.NOISE_BATCH) == (0, 1, 2)
    assert (_lib.SHEAR_33, _lib.SHEAR_KIN23, _lib.SHEAR_KCROSS23) == (0, 1, 2)
    assert (_lib.SHEAR_NOISE_HOMOSCEDASTIC, _lib.SHEAR_NOISE_33) == (0, 1)
    assert (_lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED, _lib.EHIP) == (0, -1, -2, -1000)
    assert "MGP_EINVAL" in _lib._status_message(-1) and "MGP_EUNSUPPORTED" in _lib._status_message(-2)
    assert _lib._status_message(-1001) == "HIP runtime error 1"


def test_reader_imports_without_torch():
    code = "import sys; sys.path.insert(0, %r); from muygpys_amd import _abi; assert len(_abi.signatures()) > 20; " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]

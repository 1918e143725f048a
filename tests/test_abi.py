"""The C-ABI library loads and exports every symbol include/*.h declares (no compute calls: no GPU here)."""
import ctypes
import glob
import os
import re

from conftest import ROOT


def _declared():
    names = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        src = open(h).read()
        names |= set(re.findall(r"\b(epn_[a-z0-9_]+)\s*\(", src))
    return names


def test_library_exports_every_declared_symbol():
    from epn_pointcloud_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared()
    assert len(declared) >= 14
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"
    # _lib.EXPORTS is read from the same header by the binding's own parser; _declared() is a second, cruder reading of it
    assert declared == set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) >= 188 and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


_vp, _ci, _cf, _cd, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
_ll, _i64, _u64 = ctypes.c_longlong, ctypes.c_int64, ctypes.c_uint64


def _literal_signatures(_lib):
    """Ten entry points written out by hand (from the hand-kept binding this one replaced); together they use every row of the
    type table: double, int64_t, uint64_t, long long, size_t, float, `const float *const *`, each struct pointer, (void), and
    the four return types."""
    dp, gp, tp = ctypes.POINTER(_lib.InterDesc), ctypes.POINTER(_lib.GemmNtProblem), ctypes.POINTER(_lib.GemmTnProblem)
    sp, fp = ctypes.POINTER(_lib.NormPairSide), ctypes.POINTER(_lib.NormPairFrozenSide)
    return {
        "epn_ransac_register_f64": (_ci, (_vp, _i64, _ci, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _cd, _ci, _u64, _i64, _cd, _vp, _sz,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
        "epn_fragment_pair_batch_f32": (_ci, (_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _ci, _ci, _cf, _u64, _ci, _ci,
                                              _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
        "epn_gemm_nt_f16x2_f32": (_ci, (_ci, gp, _vp, _vp, _sz, _vp)),      # a_amax, `const float *const *`: a plain pointer
        "epn_gemm_tn_grouped": (_ci, (_ci, _ci, tp, _vp, _sz, _vp)),
        "epn_norm_act_pair_frozen_fwd": (_ci, (_vp, _vp, _ci, _ll, _ci, sp, fp, _cf, _vp, _ci, _vp)),
        "epn_inter_split_saved_bytes": (_sz, (dp, _ci)),
        "epn_f16x2_overflow_count": (_ll, (_ci,)),
        "epn_version": (ctypes.c_char_p, ()),
        "epn_adam_step_f32": (_ci, (_vp, _vp, _ci, _ll, _vp, _vp, _vp, _vp, _cd, _cd, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _sz, _vp)),
        "epn_bn_running_update_f32": (_ci, (_vp, _cd, _vp, _vp, _vp, _vp, _cf, _ci, _vp)),
    }


def test_signatures_match_hand_written_ones():
    from epn_pointcloud_amd import _lib
    got = _lib.signatures()
    assert list(got) == _lib.EXPORTS
    for name, want in _literal_signatures(_lib).items():
        assert got[name] == want, name


def test_every_export_is_typed():
    """After get_lib() every declared entry point converts its arguments: none is left with ctypes' untyped default (the seven
    epn_pointnet_* calls were, before the binding was read from the header)."""
    from epn_pointcloud_amd import _lib
    cdll = _lib.get_lib()._cdll
    sigs = _lib.signatures()
    for name in _lib.EXPORTS:
        fn = getattr(cdll, name)
        assert fn.argtypes is not None, name
        assert tuple(fn.argtypes) == sigs[name][1], name
        assert fn.restype is sigs[name][0], name
    assert cdll.epn_version.argtypes == [] and len(cdll.epn_pointnet_max_f32.argtypes) == 14
    assert {r for r, _ in sigs.values()} == {_ci, _sz, _ll, ctypes.c_char_p}


def test_unwrapped_entry_points_are_the_host_only_ones():
    """The proxy hands out unwrapped exactly the declarations without an epn_stream_t parameter: the set the binding used to
    keep by hand, epn_abi_version and every *_workspace_bytes query.  Everything else comes back as the guarding wrapper."""
    import types
    from epn_pointcloud_amd import _lib
    by_hand = {"epn_inter_bwd_data_f16x2_ok", "epn_inter_ungroup_cloud_ok", "epn_inter_ungroup_cloud_range_count", "epn_version",
               "epn_strerror", "epn_set_kernel_policy", "epn_last_kernel", "epn_f16x2_overflow_count", "epn_inter_is_fused",
               "epn_inter_split_ok", "epn_inter_c1_ok", "epn_inter_split_saved_bytes", "epn_intra_is_fused", "epn_inter_onchip_ok",
               "epn_inter_group_packed_ok", "epn_inter_packed_position", "epn_adam_check_plan"}
    queries = {n for n in _lib.EXPORTS if n.endswith("_workspace_bytes")}
    assert len(queries) >= 19 and "epn_gemm_tn_workspace_bytes" in queries
    assert _lib._HOST_ONLY == by_hand | {"epn_abi_version"} | queries
    lib = _lib.get_lib()
    assert isinstance(lib.epn_gemm_nt_f32, types.FunctionType) and lib.epn_gemm_nt_f32.__name__ == "epn_gemm_nt_f32"
    assert lib.epn_gemm_nt_f32 is not lib._cdll.epn_gemm_nt_f32
    for name in ("epn_version", "epn_inter_workspace_bytes", "epn_adam_check_plan"):
        assert getattr(lib, name) is getattr(lib._cdll, name), name


def test_structs_keep_their_layout():
    """Field lists and sizes of the five Structure classes, as the hand-written classes had them."""
    from epn_pointcloud_amd import _lib
    want = {
        "InterDesc": (88, [("xyz", _vp), ("new_xyz", _vp), ("ball_idx", _vp), ("anchors", _vp), ("kernels", _vp), ("dense_w", _vp),
                           ("sigma", _cf), ("b", _ci), ("p1", _ci), ("p2", _ci), ("nn", _ci), ("na", _ci), ("ks", _ci),
                           ("cin", _ci), ("cout", _ci)]),
        "NormPairSide": (32, [("sums", _vp), ("gamma", _vp), ("beta", _vp), ("eps", _cf), ("instance", _ci)]),
        "NormPairFrozenSide": (32, [("stats", _vp), ("gamma", _vp), ("beta", _vp), ("eps", _cf), ("frozen", _ci)]),
        "GemmNtProblem": (80, [("A", _vp), ("Bt", _vp), ("C", _vp), ("M", _ll), ("lda", _ll), ("ldb", _ll), ("ldc", _ll), ("N", _ci),
                               ("K", _ci), ("col_stats", _vp), ("c_amax", _vp)]),
        "GemmTnProblem": (64, [("X", _vp), ("Y", _vp), ("C", _vp), ("R", _ll), ("ldx", _ll), ("ldy", _ll), ("ldc", _ll), ("N1", _ci),
                               ("N2", _ci)]),
    }
    for name, (size, fields) in want.items():
        cls = getattr(_lib, name)
        assert issubclass(cls, ctypes.Structure) and cls.__name__ == name
        assert cls._fields_ == fields, name
        assert ctypes.sizeof(cls) == size, name


def _parse(tmp_path, text):
    from epn_pointcloud_amd import _lib
    h = tmp_path / "synthetic.h"
    h.write_text(text)
    return _lib.parse_header(str(h))


def test_parser_refuses_a_type_it_does_not_know(tmp_path):
    """A new C type in the header must be added to the binding's table: it never falls back to a default."""
    import pytest
    with pytest.raises(RuntimeError, match="epn_odd_f32") as e:
        _parse(tmp_path, "typedef void *epn_stream_t;\nint epn_fine(int n, epn_stream_t stream);\n"
                         "int epn_odd_f32(const float *x, short n, epn_stream_t stream);\n")
    assert "short" in str(e.value) and "`n`" in str(e.value)
    with pytest.raises(RuntimeError, match="epn_odd_ret"):
        _parse(tmp_path, "float epn_odd_ret(int n);\n")
    with pytest.raises(RuntimeError, match="epn_unnamed"):
        _parse(tmp_path, "int epn_unnamed(const float *x, int);\n")
    with pytest.raises(RuntimeError, match="epn_odd_struct"):
        _parse(tmp_path, "typedef struct epn_odd_struct {\n    short n;\n} epn_odd_struct;\n")


def test_parser_reads_only_live_declarations(tmp_path):
    sigs, structs, host_only = _parse(
        tmp_path,
        "#define EPN_X(n) epn_macro(n);\n"
        "/* int epn_hidden_f32(const float *x,\n *                    epn_stream_t stream); */\n"
        "// int epn_also_hidden(int n);\n"
        "typedef struct epn_pair {\n    const void *a, *b; /* two */\n    long long n, m;\n    float w;\n} epn_pair;\n"
        "size_t epn_live_bytes(const epn_pair *p,\n                      int n); /* int epn_hidden_too(void); */\n"
        "const char *epn_name(void);\n"
        "int epn_live_f32(const float *const *xs, epn_pair *q, uint64_t seed, epn_stream_t stream);\n")
    pair = structs["epn_pair"]
    assert pair._fields_ == [("a", _vp), ("b", _vp), ("n", _ll), ("m", _ll), ("w", _cf)] and pair.__name__ == "Pair"
    assert sigs == {"epn_live_bytes": (_sz, (ctypes.POINTER(pair), _ci)), "epn_name": (ctypes.c_char_p, ()),
                    "epn_live_f32": (_ci, (_vp, ctypes.POINTER(pair), _u64, _vp))}
    assert list(sigs) == ["epn_live_bytes", "epn_name", "epn_live_f32"]
    assert host_only == {"epn_live_bytes", "epn_name"}


def test_missing_header_fails_loudly():
    import pytest
    from epn_pointcloud_amd import _lib
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "epn_so3conv.h"))
    with pytest.raises(RuntimeError, match="/nonexistent/epn_so3conv.h"):
        _lib.parse_header("/nonexistent/epn_so3conv.h")


def test_binding_loads_and_reports_version():
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    assert b"gfx950" in lib.epn_version()
    assert lib.epn_strerror(0) == b"success"
    assert b"workspace" in lib.epn_strerror(-2)


def test_workspace_query_is_host_only():
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    d = _lib.InterDesc()
    d.b, d.p1, d.p2, d.nn, d.na, d.ks, d.cin, d.cout = 2, 256, 128, 16, 60, 24, 1, 8
    d.sigma = 0.08
    n = lib.epn_inter_workspace_bytes(ctypes.byref(d))
    assert n >= 2 * 128 * 60 * 1 * 24 * 4           # generic path: grouped features are materialised


def test_packed_position_table_is_the_documented_permutation():
    """epn_inter_packed_position (host-only) against the formula in include/epn_so3conv.h, for both channel-group widths
    and a ragged second kernel-point tile; refusals for widths the packed grouping does not serve."""
    import numpy as np
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    for cin, ks in ((32, 24), (64, 24), (96, 24), (256, 24), (64, 16), (64, 12), (128, 20)):
        pos = np.full(cin * ks, -1, dtype=np.int32)
        assert lib.epn_inter_packed_position(cin, ks, pos.ctypes.data) == 0
        cg = 4 if cin % 64 == 0 else 2
        w0 = min(ks, 16)
        for c in range(cin):
            cl = c % (16 * cg)
            slot = c - cl + 16 * (cl % cg) + cl // cg
            for k in range(ks):
                want = slot * w0 + k if k < 16 else w0 * cin + slot * (ks - 16) + (k - 16)
                assert pos[c * ks + k] == want
        assert sorted(pos.tolist()) == list(range(cin * ks))
    buf = np.zeros(16 * 24, dtype=np.int32)
    assert lib.epn_inter_packed_position(16, 24, buf.ctypes.data) != 0      # cin % 32
    assert lib.epn_inter_packed_position(64, 22, buf.ctypes.data) != 0      # ks % 4
    assert lib.epn_inter_packed_position(64, 24, None) != 0


def test_missing_library_fails_loudly(monkeypatch):
    from epn_pointcloud_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libepn_so3conv.so")
    try:
        _lib.get_lib()
    except RuntimeError as e:
        assert "no CPU/eager fallback" in str(e)
    else:
        raise AssertionError("get_lib() must raise when the HIP library is missing")

"""The transposed second store's descriptor fields (kai0hip.h ct / ldct / ct2 / ldct2) on the host side, without a GPU: the ctypes
mirror matches the compiled struct, the hooks are still the descriptor's last fields, and kai0_gemm_plan — the launch's own validation
and selection, run on pointers it never follows — reports the store and refuses every combination the epilogues do not carry."""

import ctypes

import pytest


def _desc(_lib, act, M=2560, N=4096, K=256):
    d = _lib.GemmDesc()
    d.A = d.B = d.C = d.pre_out = 0x10000
    d.M, d.N, d.K, d.a_kc, d.b_kc = M, N, K, 1, 1
    d.lda = d.ldb = K
    d.ldc = N
    d.act = act
    d.ct, d.ldct = 0x20000, M
    if act == 6:
        d.B2 = d.pre_out2 = 0x10000
    else:
        d.aux1 = d.aux2 = 0x10000
        d.ct2, d.ldct2 = 0x30000, M + 8
    return d


def test_mirror_matches_the_compiled_descriptor():
    from kai0_amd import _lib

    lib = _lib.load()
    fields = [f for f, _ in _lib.GemmDesc._fields_]
    assert ctypes.sizeof(_lib.GemmDesc) == lib.kai0_gemm_desc_size()
    assert ctypes.sizeof(_lib.GemmPlan) == lib.kai0_gemm_plan_size()
    assert fields[-8:-4] == ["ct", "ldct", "ct2", "ldct2"] and fields[-4:] == ["persist", "general_epilogue", "small_w8", "_pad3"]
    assert [f for f, _ in _lib.GemmPlan._fields_][-1] == "transposed_store"


@pytest.mark.parametrize("act,persist,loop", [(6, 1, "quadrant"), (3, 1, "quadrant"), (6, 2, "persistent"), (3, 2, "persistent")])
def test_plan_reports_the_transposed_store(act, persist, loop):
    from kai0_amd import _lib

    lib = _lib.load()
    d = _desc(_lib, act, M=5120, N=8192)
    d.persist = persist
    pl = _lib.GemmPlan()
    assert lib.kai0_gemm_plan(ctypes.byref(d), ctypes.byref(pl)) == 0, lib.kai0_last_error()
    assert (pl.tile, _lib.GEMM_LOOPS[pl.loop], pl.transposed_store) == (256, loop, 1)
    d.ct = d.ct2 = None
    assert lib.kai0_gemm_plan(ctypes.byref(d), ctypes.byref(pl)) == 0 and pl.transposed_store == 0


def test_what_the_epilogues_do_not_carry_is_refused():
    from kai0_amd import _lib

    lib = _lib.load()
    pl = _lib.GemmPlan()

    def refused(d, msg):
        assert lib.kai0_gemm_plan(ctypes.byref(d), ctypes.byref(pl)) != 0, msg
        assert msg.encode() in lib.kai0_last_error(), (msg, lib.kai0_last_error())

    for act in (6, 3):
        assert lib.kai0_gemm_plan(ctypes.byref(_desc(_lib, act)), ctypes.byref(pl)) == 0, lib.kai0_last_error()
    d = _desc(_lib, 0)
    d.ct2, d.pre_out, d.aux1, d.aux2 = None, None, None, None
    assert lib.kai0_gemm_plan(ctypes.byref(d), ctypes.byref(pl)) == 0 and pl.transposed_store == 1, lib.kai0_last_error()
    d = _desc(_lib, 3)
    d.split_k, d.workspace, d.workspace_bytes = 2, 0x40000, 2 * 2560 * 4096 * 4
    refused(d, "transposed store excludes")
    d = _desc(_lib, 3)
    d.c_rpb, d.c_bs = 512, 1024
    refused(d, "transposed store excludes")
    d = _desc(_lib, 3)
    d.batch = 2
    refused(d, "transposed store excludes")
    d = _desc(_lib, 1)
    d.ct2 = None
    refused(d, "needs act=0 or act=6 with ct")
    d = _desc(_lib, 0)  # (ct2 set: act 0 takes ct alone)
    refused(d, "needs act=0 or act=6 with ct")
    d = _desc(_lib, 0)
    d.ct2, d.pre_out, d.aux1, d.aux2, d.bias = None, None, None, None, 0x10000
    refused(d, "plain form")
    d = _desc(_lib, 6)
    d.ct2, d.ldct2 = 0x30000, 2560
    refused(d, "needs act=0 or act=6 with ct")
    d = _desc(_lib, 3)
    d.ct2 = None
    refused(d, "needs act=0 or act=6 with ct")
    d = _desc(_lib, 3)
    d.ct = None
    refused(d, "needs act=0 or act=6 with ct")
    for field, bad in (("ldct", 2560 + 4), ("ldct", 2552), ("ldct2", 2560 + 2), ("ct", 0x20008)):
        d = _desc(_lib, 3)
        setattr(d, field, bad)
        refused(d, "ldct % 8 == 0")
    d = _desc(_lib, 3, M=2556)
    refused(d, "M % 8 == 0")
    d = _desc(_lib, 3)
    d.residual, d.ldr = 0x10000, 4096
    refused(d, "plain form")
    d = _desc(_lib, 3, M=1024)
    refused(d, "256 x 256")
    d = _desc(_lib, 3)
    d.out_f32 = 1
    assert lib.kai0_gemm_plan(ctypes.byref(d), ctypes.byref(pl)) != 0
    d = _desc(_lib, 3)
    d.nseg = 1
    d.seg[0].dst, d.seg[0].ld = 0x10000, 4096
    assert lib.kai0_gemm_plan(ctypes.byref(d), ctypes.byref(pl)) != 0

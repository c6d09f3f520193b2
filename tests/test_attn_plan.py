"""CPU: which kernel every launch of ur_attn_fwd / ur_attn_bwd takes, as the library's one selection function answers it
(ur_attn_plan -> hip.attn_plan; no device, nothing is launched).  The case list of tests/attn_cases.py reaches every kernel; the
few-query workspace query, the generated backward pair and the tiny backward obey their all-or-nothing rules on a grid of boundary
sizes; the smallest shapes on each side of every selection boundary, mode on and off; the query refuses what the entry points refuse."""
import ctypes
import itertools

import pytest

from tests import attn_cases as ac
from unirec_amd import _lib, hip

SIZES = (1, 2, 4, 5, 16, 17, 32, 33, 64, 65, 127, 128, 129, 192, 255, 256, 257, 384, 520, 576, 640, 4096, 4160, 8192)


def _plan(Sq, Sk, hd, causal, nq=1, nkv=1, B=1, p=0.0, modes=(), fwd_only=False):
    a, g = ac.plan_args(B, Sq, Sk, nq, nkv, hd, causal, p)
    return ac.plan_of(a, None if fwd_only else g, modes)


def _ids(*args, **kw):
    pl = _plan(*args, **kw)
    return pl["fwd"], pl["dq"], pl["dkv"]


def test_the_case_list_reaches_every_kernel():
    """docs/lab_notes.md section 17 (Coverage): over the 204 cases, each under its own modes, every forward, dQ and dK/dV kernel id
    occurs, and every kernel name the Python layer knows is one of them"""
    seen = {"fwd": set(), "dq": set(), "dkv": set()}
    cases = ac.all_cases()
    assert len(cases) == 204
    for c in cases:
        pl = ac.plan(c)
        for launch in seen:
            seen[launch].add(pl[launch])
    assert seen["fwd"] == {"generic", "c128", "tiny"}
    assert seen["dq"] == {"generic", "c128", "tiny"}
    assert seen["dkv"] == {"generic", "dkv2", "fewq", "c128", "tiny"}
    assert {k for k in hip.ATTN_KERNELS if k is not None} - {"none"} == seen["fwd"] | seen["dq"] | seen["dkv"]


def test_colsum_workspace_query_is_the_plans_fewq_answer():
    """ur_attn_bwd_kv_colsum_floats(a) > 0 exactly when the plan's dK/dV kernel is fewq: head_dim 64, non-causal, every (Sq, Sk) of the
    boundary sizes, every GQA ratio, B 1 / 3 without / with dropout, all 4 x 2 x 2 x 2 mode settings"""
    lib, out, FEWQ = _lib.load(), _lib.AttnPlanInfo(), hip.ATTN_KERNELS.index("fewq")
    n = 0
    for tiny, c128, pers, fewq in itertools.product(range(4), range(2), range(2), range(2)):
        with ac.plan_modes((("TINY", tiny), ("C128", c128), ("DKV_PERSIST", pers), ("FEWQ", fewq))):
            for (nq, nkv), (B, p) in itertools.product(ac.HEADS, ((1, 0.0), (3, 0.1))):
                a, g = ac.plan_args(B, 1, 1, nq, nkv, 64, False, p)
                a.q = a.k = a.v = a.stats = 4096      # the size query wants operands (non-null, 16-byte aligned); it never reads them
                pa, pg, pout = ctypes.byref(a), ctypes.byref(g), ctypes.byref(out)
                for Sq, Sk in itertools.product(SIZES, SIZES):
                    a.Sq, a.Sk = Sq, Sk
                    words = lib.ur_attn_bwd_kv_colsum_floats(pa)
                    assert lib.ur_attn_plan(pa, pg, pout) == 0      # (hip.attn_plan without its dict: 147 456 queries)
                    is_fewq = out.dkv == FEWQ
                    assert words == (2 * B * nq * 64 if is_fewq else 0), (Sq, Sk, nq, nkv, B, tiny, c128, pers, fewq, words)
                    n += is_fewq
    assert n > 0


def test_backward_pair_and_tiny_are_all_or_nothing():
    """the generated dQ and dK/dV kernels share the -LSE2 plane: dq is c128 exactly when dkv is, and lse_log2 is set exactly then; the
    tiny backward is one kernel: dq is tiny exactly when dkv is.  Both head_dims; causal S x S and non-causal Sq x Sk over the boundary
    sizes; every GQA ratio; B 1 / 3 without / with dropout; TINY x C128 x FEWQ"""
    n_pair = n_tiny = 0
    shapes = [(hd, True, S, S) for hd in (64, 128) for S in SIZES]
    shapes += [(hd, False, Sq, Sk) for hd in (64, 128) for Sq in (1, 4, 5, 32, 33, 64, 65, 128, 256, 4096) for Sk in SIZES]
    for tiny, c128, fewq in itertools.product(range(4), range(2), range(2)):
        with ac.plan_modes((("TINY", tiny), ("C128", c128), ("FEWQ", fewq))):
            for (nq, nkv), (B, p) in itertools.product(ac.HEADS, ((1, 0.0), (3, 0.1))):
                for hd, causal, Sq, Sk in shapes:
                    if causal and p > 0:
                        continue      # (refused: test_the_query_refuses_what_the_entry_points_refuse)
                    pl = hip.attn_plan(*ac.plan_args(B, Sq, Sk, nq, nkv, hd, causal, p))
                    assert (pl["dq"] == "c128") == (pl["dkv"] == "c128") == bool(pl["lse_log2"]), (hd, causal, Sq, Sk, nq, nkv, B, p, pl)
                    assert (pl["dq"] == "tiny") == (pl["dkv"] == "tiny"), (hd, causal, Sq, Sk, nq, nkv, B, p, pl)
                    assert pl["dq"] != "c128" or pl["fwd"] == "c128", pl
                    n_pair += pl["dq"] == "c128"
                    n_tiny += pl["dq"] == "tiny"
    assert n_pair > 0 and n_tiny > 0


def test_tiny_boundary():
    G3 = ("generic",) * 3
    assert _ids(4, 16, 64, False) == ("tiny",) * 3
    assert _ids(5, 16, 64, False) == G3 and _ids(4, 17, 64, False) == G3
    assert _ids(4, 16, 64, False, nq=2, nkv=1) == G3 and _ids(4, 4, 64, True) == G3 and _ids(4, 16, 128, False) == G3
    assert _ids(4, 16, 64, False, modes=(("TINY", 0),)) == G3
    assert _ids(4, 16, 64, False, modes=(("TINY", 1),)) == ("tiny", "generic", "generic")
    assert _ids(4, 16, 64, False, modes=(("TINY", 2),)) == ("generic", "tiny", "tiny")


def test_fewq_boundary():
    assert _ids(64, 256, 64, False) == ("generic", "generic", "fewq")
    assert _ids(64, 256, 64, False, nq=3, nkv=3, B=3, p=0.1) == ("generic", "generic", "fewq")
    assert _ids(64, 255, 64, False)[2] == "generic" and _ids(65, 256, 64, False)[2] == "generic"
    assert _ids(64, 256, 64, False, nq=2, nkv=1)[2] == "generic"
    assert _ids(64, 256, 128, False)[2] == "dkv2" and _ids(256, 256, 64, True)[2] == "generic"
    assert _ids(64, 256, 64, False, modes=(("FEWQ", 0),)) == ("generic",) * 3
    assert _ids(1, 8192, 64, False)[2] == "fewq"


def test_generated_kernel_boundaries():
    """whole 64-key tiles from 128 keys for the forward, whole 128-key blocks for the backward pair (192: generated forward, generic
    backward), MAX_SK = 4096, and UR_ATTN_MODE_C128 = 0"""
    off = (("C128", 0),)
    assert _ids(64, 64, 128, True) == ("generic",) * 3
    assert _ids(128, 128, 128, True) == ("c128",) * 3 and _plan(128, 128, 128, True)["lse_log2"] == 1
    assert _ids(192, 192, 128, True) == ("c128", "generic", "dkv2") and _plan(192, 192, 128, True)["lse_log2"] == 0
    assert _ids(576, 576, 128, True, nq=4, nkv=1, B=3) == ("c128", "generic", "dkv2")
    assert _ids(256, 256, 128, True) == ("c128",) * 3
    assert _ids(129, 129, 128, True) == ("generic", "generic", "dkv2") and _ids(128, 128, 64, True) == ("generic",) * 3
    assert _ids(4096, 4096, 128, True, nq=4, nkv=2) == ("c128",) * 3
    assert _ids(4160, 4160, 128, True, nq=4, nkv=2) == ("generic", "generic", "dkv2")
    for S in (128, 192, 256, 4096):
        assert _ids(S, S, 128, True, modes=off) == ("generic", "generic", "dkv2") and _plan(S, S, 128, True, modes=off)["lse_log2"] == 0
    # the forward alone: nothing of the backward is selected
    assert _plan(128, 128, 128, True, fwd_only=True) == dict(fwd="c128", dq="none", dkv="none", lse_log2=0, nw_q=4, nw_k=4)
    assert _ids(128, 128, 128, True, B=0) == ("none",) * 3


def test_dropout_boundary():
    """attn_bwd_dkv2_kernel draws no dropout: head_dim 128, non-causal, 0 against 0.1"""
    assert _ids(128, 128, 128, False) == ("generic", "generic", "dkv2")
    assert _ids(128, 128, 128, False, p=0.1) == ("generic",) * 3


@pytest.mark.parametrize("S,nw", [(32, 1), (33, 2), (64, 2), (65, 4)])
def test_nw_thresholds(S, nw):
    """waves per workgroup of the generic kernels: by queries for the forward and dQ, by keys for dK/dV (whose 4-wave head_dim-128
    launches without dropout are attn_bwd_dkv2_kernel)"""
    for hd, causal in itertools.product((64, 128), (False, True)):
        pl = _plan(S, S, hd, causal)
        assert (pl["nw_q"], pl["nw_k"]) == (nw, nw) and (pl["fwd"], pl["dq"]) == ("generic", "generic")
        assert pl["dkv"] == ("dkv2" if hd == 128 and nw == 4 else "generic")
    pl = _plan(S, 100, 128, False)
    assert (pl["nw_q"], pl["nw_k"], pl["dkv"]) == (nw, 4, "dkv2")
    pl = _plan(100, S, 128, False)
    assert (pl["nw_q"], pl["nw_k"], pl["dkv"]) == (4, nw, "dkv2" if nw == 4 else "generic")


@pytest.mark.parametrize("kw,text", [
    (dict(hd=96), "head_dim must be 64 or 128"),
    (dict(nq=3, nkv=2), "bad sizes"),
    (dict(causal=True, Sq=64, Sk=128), "causal mode needs Sq == Sk"),
    (dict(Sk=8256), "exceeds 8192"),
    (dict(causal=True, Sq=128, p=0.1), "bad dropout"),
    (dict(scale=0.0), "scale must be positive"),
    (dict(scale=-1.0), "scale must be positive"),
])
def test_the_query_refuses_what_the_entry_points_refuse(kw, text):
    args = dict(B=2, Sq=128, Sk=128, nq=2, nkv=2, hd=64, causal=False, p=0.0, scale=None)
    args.update(kw)
    a, g = ac.plan_args(**args)
    for bwd in (None, g):
        with pytest.raises(_lib.UniRecHipError, match=text):
            hip.attn_plan(a, bwd)
    # ... and a kv_colsum request on a shape whose dK/dV kernel is not the few-query one, as ur_attn_bwd does
    a, g = ac.plan_args(2, 128, 128, 2, 2, 64, False)
    g.kv_colsum = 4096
    with pytest.raises(_lib.UniRecHipError, match="few-query dK/dV kernel only"):
        hip.attn_plan(a, g)
    a.Sq, a.Sk = 64, 256
    assert hip.attn_plan(a, g)["dkv"] == "fewq"

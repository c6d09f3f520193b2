"""CPU: the host side of streaming catalogue retrieval -- pack_exclude, ranking_metrics, and the argument checks and the size query
of ur_catalog_scores' select mode through the raw library (fake non-null pointers: every call here returns before any launch)."""
import ctypes
import math

import pytest
import torch

from unirec_amd import _lib
from unirec_amd.evaluation import pack_exclude, ranking_metrics

FAKE = 256          # non-null, 16-byte aligned, never dereferenced on the host


# ---- pack_exclude -------------------------------------------------------------------------------------------------------------
def _members(row):
    return {int(v) for v in row.tolist() if v >= 0}


def test_pack_exclude_ragged_lists():
    ragged = [[9, 2, 5], [], [4], (7, 7, 1), range(3)]
    t = pack_exclude(ragged)
    assert t.dtype == torch.int64 and t.shape == (5, 3) and t.is_contiguous()
    for row, src in zip(t, ragged):
        assert torch.equal(row, torch.sort(row).values), "rows are ascending (the kernel binary-searches them)"
        assert _members(row) == set(src), "membership is preserved"
        assert all(int(v) == -1 for v in row[row < 0]), "empty slots are -1"
        n_neg = int((row < 0).sum())
        assert bool((row[:n_neg] < 0).all()) and bool((row[n_neg:] >= 0).all()), "empty slots sort first"
    assert t[0].tolist() == [2, 5, 9] and t[1].tolist() == [-1, -1, -1] and t[2].tolist() == [-1, -1, 4]


def test_pack_exclude_padded_tensor():
    src = torch.tensor([[5, -1, 3, 3], [-1, -1, -1, -1], [0, 8, -7, 2]], dtype=torch.int64)
    t = pack_exclude(src)
    assert t.dtype == torch.int64 and t.shape == (3, 4)
    assert t.tolist() == [[-1, 3, 3, 5], [-1, -1, -1, -1], [-1, 0, 2, 8]]
    assert src.tolist() == [[5, -1, 3, 3], [-1, -1, -1, -1], [0, 8, -7, 2]], "the input is left alone"


def test_pack_exclude_nothing_excluded_is_none():
    assert pack_exclude(None) is None
    assert pack_exclude([]) is None
    assert pack_exclude([[], [], ()]) is None
    assert pack_exclude(torch.full((4, 3), -1, dtype=torch.int64)) is None
    assert pack_exclude(torch.empty((4, 0), dtype=torch.int64)) is None


def test_pack_exclude_checks_the_user_count():
    assert pack_exclude([[1], [2]], num_users=2).shape == (2, 1)
    with pytest.raises(ValueError):
        pack_exclude([[1], [2]], num_users=3)


# ---- ranking_metrics ----------------------------------------------------------------------------------------------------------
def test_ranking_metrics_closed_forms():
    ranks, ks = [1, 2, 3, 11], (1, 10)
    m = ranking_metrics(torch.tensor(ranks, dtype=torch.int32), ks)
    assert m.dtype == torch.float64 and m.shape == (1 + 2 * len(ks),)
    want = [sum(1.0 / r for r in ranks) / 4]
    want += [sum(r <= k for r in ranks) / 4 for k in ks]
    want += [sum(1.0 / math.log2(1 + r) if r <= k else 0.0 for r in ranks) / 4 for k in ks]
    assert want[1:3] == [0.25, 0.75]
    for got, ref in zip(m.tolist(), want):
        assert abs(got - ref) <= 4 * 2.0 ** -52 * max(abs(ref), 1.0), (got, ref)      # float64 means of four terms


# ---- ur_catalog_scores, select mode: checks and size query --------------------------------------------------------------------
def _select(**over):
    s = _lib.CatalogSelect()
    s.K, s.E = 10, 0
    s.topk_index = s.topk_score = FAKE
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _call(lib, sel, B=4, N=5000, D=16, scores=None):
    return lib.ur_catalog_scores(FAKE, FAKE, scores, FAKE, FAKE, 0, B, N, D, None if sel is None else ctypes.byref(sel), None)


def _query(lib, **kw):
    s = _select()
    assert _call(lib, s, **kw) == 0
    return s.workspace_bytes


def test_size_query_writes_the_bytes_and_launches_nothing():
    lib = _lib.load()
    s = _select(workspace_bytes=-7)
    assert _call(lib, s) == 0
    assert s.workspace_bytes > 0
    # default chunk: the whole (small) catalogue rounded up to the 1024-score tile, for every user, plus the per-user reference scores
    assert s.workspace_bytes >= 4 * 5120 * 4 + 4 * 4
    assert s.workspace_bytes < 4 * 5120 * 4 + 4096
    # a caller's chunk_rows sizes the buffer; more rows than the catalogue has are not paid for
    s2 = _select(chunk_rows=1024)
    assert _call(lib, s2) == 0 and 4 * 1024 * 4 <= s2.workspace_bytes < 4 * 1024 * 4 + 4096
    s3 = _select(chunk_rows=1 << 20)
    assert _call(lib, s3) == 0 and s3.workspace_bytes == s.workspace_bytes
    # at catalogue scale the default chunk buffer stays near 64 MB, whatever N is
    big = _select()
    assert _call(lib, big, B=512, N=4_000_000, D=1024) == 0
    assert 32 << 20 <= big.workspace_bytes <= (64 << 20) + 4096
    assert big.workspace_bytes < 512 * 4_000_000


def test_select_argument_checks_reject_without_launching():
    lib = _lib.load()
    need = _query(lib)

    def rejected(sel, **kw):
        rc = _call(lib, sel, **kw)
        msg = lib.ur_last_error()
        assert rc < 0 and b"ur_catalog_scores" in msg, (rc, msg)

    ok = dict(workspace=FAKE, workspace_bytes=need)
    rejected(_select(K=0, **ok))
    rejected(_select(K=129, **ok))
    rejected(_select(K=0))                                               # (a size query checks the sizes too)
    rejected(_select(**ok), N=2 ** 31)
    rejected(_select(gt_index=FAKE, **ok))                               # gt_index without rank
    rejected(_select(rank=FAKE, **ok))                                   # rank without gt_index
    rejected(_select(E=3, **ok))                                         # E > 0 with exclude NULL
    rejected(_select(E=-1, exclude=FAKE, **ok))
    rejected(_select(chunk_rows=1000, **ok))
    rejected(_select(chunk_rows=-1024, **ok))
    rejected(_select(workspace=FAKE, workspace_bytes=need - 1))          # one byte short
    rejected(_select(workspace=FAKE + 4, workspace_bytes=need + 64))     # misaligned
    rejected(_select(topk_index=None, **ok))
    rejected(_select(**ok), D=6)
    # K = 128 and N = 2**31 - 1 are inside the limits: their size queries succeed
    assert _call(lib, _select(K=128)) == 0
    assert _call(lib, _select(), N=2 ** 31 - 1) == 0


def test_wrapper_refuses_mismatched_operands_before_the_library(monkeypatch):
    """shapes that the library would read out of bounds: a ValueError under the wrapper's name, on host tensors, nothing loaded"""
    from unirec_amd import hip

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    user, cat = torch.zeros(2, 16), torch.zeros(5, 16)
    for args, kw in (((torch.zeros(16), cat), {}),
                     ((user, torch.zeros(5, 4, 4)), {}),
                     ((user, torch.zeros(5, 12)), {}),
                     ((user, cat), dict(cat_inv_norm=torch.ones(4))),
                     ((user, cat), dict(cat_inv_norm=torch.ones(5, dtype=torch.float64)))):
        with pytest.raises(ValueError, match="catalog_select"):
            hip.catalog_select(*args, 3, **kw)


def test_workspace_layouts_under_the_host_sanitizers(tmp_path):
    """tests/host/catalog_layout_check.cpp: every catalogue workspace over a grid of sizes -- regions aligned, disjoint and inside the
    size the query answers, the size the closed form -- as a stand-alone host program under AddressSanitizer and UBSan"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the sanitizer runtimes are linked statically: a dynamic one insists on being the first library the process loads
    gxx, clang = shutil.which("g++"), shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang, "-static-libsan"]
    exe = str(tmp_path / "catalog_layout_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(root, "unirec_amd", "csrc"), os.path.join(root, "tests", "host", "catalog_layout_check.cpp"), "-o", exe],
                   check=True)
    # (the program allocates nothing it does not free at exit; the leak pass needs ptrace, which a sandbox may not grant)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.split() == ["ok", "648"], (run.returncode, run.stdout, run.stderr)


def test_plain_call_still_needs_scores():
    lib = _lib.load()
    rc = _call(lib, None, scores=None)
    assert rc < 0 and b"ur_catalog_scores" in lib.ur_last_error() and b"null" in lib.ur_last_error()

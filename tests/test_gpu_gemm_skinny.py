"""gemm_bt_skinny (gemm_skinny.hip, 64x64 tiles) against the two existing
MFMA GEMMs.

All three kernels feed every 16x16 output fragment through ONE accumulator
chain of v_mfma_f32_16x16x32_bf16 over K ascending in steps of 32 and share
the store_frag epilogue, so the comparison is torch.equal, not a tolerance.
"""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

RING = 4  # SK_RING of gemm_skinny.hip


@pytest.fixture(scope="module")
def hip():
    from mcp_context_forge_amd.ops import hip as _hip

    if not _hip.available():
        pytest.fail("libforge_hip must load on a GPU box (no silent fallback)")
    return _hip


def _operands(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(m, k, generator=g) * 0.5).to(torch.bfloat16).cuda()
    bt = (torch.randn(n, k, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return a, bt


def _v1(hip, monkeypatch, *args, **kw):
    monkeypatch.setenv("FORGE_GEMM_V1", "1")
    try:
        return hip.gemm_bt(*args, **kw)
    finally:
        monkeypatch.delenv("FORGE_GEMM_V1", raising=False)


@pytest.mark.parametrize("m,n,k", [
    (128, 128, 64),                  # one K step
    (128, 256, 128),                 # two N tiles, two K steps
    (256, 128, 64 * (RING + 2)),     # wraps the LDS ring and drains
    (128, 1024, 4096),               # the rescan shape
])
def test_skinny_equals_v1(hip, monkeypatch, m, n, k):
    a, bt = _operands(m, n, k, seed=m + n + k)
    want = _v1(hip, monkeypatch, a, bt)
    got = hip.gemm_bt_skinny(a, bt)
    assert torch.equal(got, want)


@pytest.mark.parametrize("m,n,k", [(256, 256, 96 * 2), (1024, 1024, 4096)])
def test_skinny_equals_v2(hip, monkeypatch, m, n, k):
    monkeypatch.delenv("FORGE_GEMM_V1", raising=False)
    a, bt = _operands(m, n, k, seed=7 + m)
    want = hip.gemm_bt(a, bt)   # the dispatcher picks v2 for these shapes
    got = hip.gemm_bt_skinny(a, bt)
    assert torch.equal(got, want)


def test_m64_is_the_top_half_of_m128(hip):
    a, bt = _operands(128, 128, 256, seed=3)
    full = hip.gemm_bt_skinny(a, bt)
    half = hip.gemm_bt_skinny(a[:64].contiguous(), bt)
    assert half.shape == (64, 128)
    assert torch.equal(half, full[:64])


@pytest.mark.parametrize("act", ["none", "gelu", "sigmoid"])
@pytest.mark.parametrize("out_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_epilogue_matrix_equals_v1(hip, monkeypatch, act, out_bf16, has_bias):
    code = {"none": hip.ACT_NONE, "gelu": hip.ACT_GELU, "sigmoid": hip.ACT_SIGMOID}[act]
    a, bt = _operands(128, 128, 128, seed=11)
    bias = torch.linspace(-1.0, 1.0, 128).cuda() if has_bias else None
    want = _v1(hip, monkeypatch, a, bt, bias, act=code, out_bf16=out_bf16)
    got = hip.gemm_bt_skinny(a, bt, bias, act=code, out_bf16=out_bf16)
    assert got.dtype == want.dtype
    assert torch.equal(got, want)


@pytest.mark.parametrize("m,n,k", [(96, 128, 64), (128, 96, 64), (128, 128, 32), (128, 128, 96),
                                   (0, 128, 64)])
def test_bad_shape_is_refused_and_writes_nothing(hip, m, n, k):
    a = torch.ones(max(m, 1), k, dtype=torch.bfloat16, device="cuda")
    bt = torch.ones(n, k, dtype=torch.bfloat16, device="cuda")
    c = torch.full((max(m, 1), n), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = hip._load().forge_gemm_bt_skinny(p(a), p(bt), ctypes.c_void_p(0), p(c), m, n, k,
                                          hip.ACT_NONE, 0, hip._stream())
    assert rc == hip.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((c == 7.0).all())


def test_classifier_routes_small_batches_to_skinny(hip, monkeypatch):
    """GpuClassifier picks the skinny kernel up to SKINNY_MAX_M rows and
    gemm_bt above it or with FORGE_GEMM_SKINNY=0; hip.gemm_bt itself is not
    rerouted."""
    from mcp_context_forge_amd.gpu import classifier as C

    clf = C.GpuClassifier.__new__(C.GpuClassifier)
    clf.dim, clf.hidden, clf.classes = 4096, 1024, 8
    monkeypatch.delenv("FORGE_GEMM_SKINNY", raising=False)
    assert clf._gemm(128) is hip.gemm_bt_skinny
    assert clf._gemm(C.SKINNY_MAX_M) is hip.gemm_bt_skinny
    assert clf._gemm(C.SKINNY_MAX_M + 128) is hip.gemm_bt
    monkeypatch.setenv("FORGE_GEMM_SKINNY", "0")
    assert clf._gemm(128) is hip.gemm_bt

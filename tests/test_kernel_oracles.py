"""The oracles and inputs of tests/test_gpu_dense.py, checked without a GPU:
a wrong oracle or a degenerate input would make the GPU tests pass for the
wrong reason."""

import numpy as np
import pytest
import torch

import kernel_oracles as ko
from mcp_context_forge_amd.ops import dfa
from mcp_context_forge_amd.ops.featurize import featurize_batch


# ---- integer cases --------------------------------------------------------

@pytest.mark.parametrize("kernel,m,n,k", ko.GEMM_CASES)
def test_integer_gemm_case_is_exact_and_not_degenerate(kernel, m, n, k):
    a, bt, bias, ref, ref_b = ko.int_gemm_case(m, n, k)
    for t in (a, bt):
        v = t.float()
        assert torch.equal(v, v.round()) and v.abs().max().item() == 4 and v.min().item() == -4
    assert bias.abs().max().item() <= 6 and torch.equal(bias, bias.round())
    # every partial sum of every accumulation order is an integer below 2^24
    bound = (a.to(torch.int64).abs() @ bt.to(torch.int64).abs().t()).max().item() + 6
    assert bound < 2 ** 24
    assert max(ref.abs().max().item(), ref_b.abs().max().item()) <= bound
    # the int64 reference is the float64 one
    assert torch.equal(ref.double(), ko.gemm_ref(a, bt))
    assert torch.equal(ref_b.double(), ko.gemm_ref(a, bt, bias))
    # a transposed, permuted or repeated row / column block changes the result
    assert len({tuple(r) for r in ref.tolist()}) == m
    assert len({tuple(c) for c in ref.t().tolist()}) == n
    assert len({tuple(r) for r in a.float().tolist()}) == m
    assert len({tuple(r) for r in bt.float().tolist()}) == n
    if m == n:
        assert not torch.equal(ref, ref.t())
    # no 32-wide K block repeats inside a row, so a K step read twice shows
    if k >= 64:
        blocks = a.float().view(m, k // 32, 32)
        assert not torch.equal(blocks[:, 0], blocks[:, 1])


@pytest.mark.parametrize("kernel,m,n,k", ko.GEMM_CASES)
def test_integer_bf16_case_holds_ties_both_ways(kernel, m, n, k):
    _, _, _, ref, ref_b = ko.int_gemm_case(m, n, k)
    for r in (ref, ref_b):
        f32 = r.float()
        assert torch.equal(f32.to(torch.int64), r)
        down, up = ko.bf16_tie_counts(f32)
        assert down > 0 and up > 0, (down, up)
        # torch's conversion is round-to-nearest-even: it differs from truncation on the "up" ties
        trunc = (f32.view(torch.int32) & -65536).view(torch.float32)
        assert int((f32.bfloat16().float() != trunc).sum()) >= up


def test_bf16_tie_counts():
    x = torch.tensor([256.0, 257.0, 259.0, -257.0, -259.0, 258.0, 514.0, 518.0, 1.0])
    assert ko.bf16_tie_counts(x) == (3, 3)
    assert x.bfloat16().float().tolist() == [256.0, 256.0, 260.0, -256.0, -260.0, 258.0, 512.0, 520.0, 1.0]


@pytest.mark.parametrize("m,c,k", ko.GEMV_SHAPES)
def test_integer_gemv_case(m, c, k):
    a, wt, bias, ref, ref_b = ko.int_gemm_case(m, c, k)
    assert (a.to(torch.int64).abs() @ wt.to(torch.int64).abs().t()).max().item() + 6 < 2 ** 24
    assert ref.shape == (m, c) and not torch.equal(ref, ref_b)


@pytest.mark.parametrize("d", ko.VERIFY_DOT_D)
@pytest.mark.parametrize("m", ko.VERIFY_DOT_M)
def test_integer_verify_dot_case(m, d):
    feats, keys, idx, ref = ko.int_verify_dot_case(m, d)
    idx = idx.numpy()
    assert 16 * d < 2 ** 24 and idx.min() >= -1 and idx.max() < keys.shape[0]
    assert (idx < 0).any() or m == 1
    assert (ref[idx < 0] == ko.SENTINEL).all()
    for i in np.nonzero(idx >= 0)[0]:
        assert ref[i] == float(feats[i].double() @ keys[idx[i]].double())
    if d > 8:   # the last 8-element chunk matters: dropping it changes every dot
        short = feats[:, :d - 8].to(torch.int64) @ keys[:, :d - 8].to(torch.int64).t()
        for i in np.nonzero(idx >= 0)[0]:
            assert short[i, idx[i]].item() != ref[i]


def test_verify_dot_cases_hold_a_missing_candidate():
    assert any((ko.int_verify_dot_case(m, 512)[2].numpy() < 0).any() for m in ko.VERIFY_DOT_M)


# ---- float64 GEMM oracle and bounds ---------------------------------------

def test_gemm_ref_and_abs_dot_against_a_python_loop():
    a, bt = ko.random_operands(3, 4, 5, seed=1)
    bias = torch.tensor([0.5, -1.0, 2.0, 0.0])
    import math

    for act in ko.ACTS:
        got = ko.gemm_ref(a, bt, bias, act)
        for i in range(3):
            for j in range(4):
                z = sum(float(a[i, k]) * float(bt[j, k]) for k in range(5)) + float(bias[j])
                want = {"none": z,
                        "gelu": 0.5 * z * (1 + math.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3))),
                        "sigmoid": 1 / (1 + math.exp(-z))}[act]
                assert abs(got[i, j].item() - want) <= 1e-15 * max(1.0, abs(want))
    ad = ko.abs_dot(a, bt)
    assert ad[1, 2].item() == pytest.approx(sum(abs(float(a[1, k])) * abs(float(bt[2, k])) for k in range(5)), rel=1e-15)
    # the float64 GELU is torch's own tanh GELU
    z = torch.linspace(-6, 6, 101, dtype=torch.float64)
    assert torch.allclose(ko.act_ref(z, "gelu"), torch.nn.functional.gelu(z, approximate="tanh"), rtol=0, atol=1e-15)


@pytest.mark.parametrize("kernel,m,n,k", ko.GEMM_CASES)
def test_working_bound_tells_fp32_from_a_bf16_round_trip(kernel, m, n, k):
    """MARGIN x the measured error stays below half a bf16 ulp of |ref| where
    |ref| >= 1, and below the derived hard bound."""
    _, _, ref, ad = ko.random_gemm_case(kernel, m, n, k)
    big = ref.abs() >= 1.0
    assert int(big.sum()) > ref.numel() // 4
    assert bool((ko.gemm_working_bound(kernel) * ad[big] < ko.BF16_HALF_ULP * ref.abs()[big]).all())
    assert ko.gemm_working_bound(kernel) <= k * ko.GEMM_HARD_EPS or k < 64
    # a result rounded through bf16 would be caught on some element
    through = ref.float().bfloat16().double()
    assert bool(((through - ref).abs() > ko.gemm_working_bound(kernel) * ad).any())


@pytest.mark.parametrize("kernel", sorted(ko.EPILOGUE_SHAPES))
@pytest.mark.parametrize("act", ko.ACTS)
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_no_other_epilogue_wiring_can_pass(kernel, act, has_bias):
    """test_gemm_epilogue_matrix's separation, at the new shapes and the new
    (tighter) tolerance: every other (act, bias) reference is >= 4 tolerances away."""
    a, bt, _, refs = ko.epilogue_case(kernel)
    k = a.shape[1]
    ad = ko.abs_dot(a, bt)
    # the widest tolerance any new check of this combination uses
    tol = ko.epilogue_tol(k * ko.GEMM_HARD_EPS, ad, refs[("none", has_bias)], "gemm", act)
    assert ko.wiring_separation(refs, (act, has_bias), tol) >= 1.0


@pytest.mark.parametrize("m,c,k", ko.GEMV_SHAPES)
@pytest.mark.parametrize("act", ko.ACTS)
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_no_other_gemv_wiring_can_pass(m, c, k, act, has_bias):
    a, wt, _, refs = ko.gemv_case(m, c, k)
    ad = ko.abs_dot(a, wt)
    tol = ko.epilogue_tol(k * ko.DOT_EPS, ad, refs[("none", has_bias)], "gemv", act)
    assert ko.wiring_separation(refs, (act, has_bias), tol) >= 1.0


# ---- rows_argmax_merge ----------------------------------------------------

def _merge_loop(scores, valid, idx_base, best_val, best_idx):
    bv, bi = best_val.copy(), best_idx.copy()
    for r in range(scores.shape[0]):
        mx, arg = ko.SENTINEL, -1
        for c in range(scores.shape[1]):
            x = scores[r, c] if valid is None or valid[c] else ko.SENTINEL
            if x > mx:
                mx, arg = x, c
        if arg >= 0 and mx > bv[r]:
            bv[r], bi[r] = mx, idx_base + arg
    return bv, bi


@pytest.mark.parametrize("nc", [1, 3, 4, 9, 70])
@pytest.mark.parametrize("kind", ["none", "random", "ones", "zeros"])
def test_argmax_merge_ref_equals_a_python_loop(nc, kind):
    m = 6
    scores = ko.argmax_scores(m, nc, seed=nc)
    buf = ko.argmax_valid(kind, nc, seed=nc + 1)
    valid = None if buf is None else buf[ko.VALID_OFFSET:ko.VALID_OFFSET + nc]
    carried_v = np.array([ko.SENTINEL, 1.0, 3.75, 100.0, ko.SENTINEL, 0.25], dtype=np.float32)
    carried_i = np.array([-1, 7, 8, 9, -1, 3], dtype=np.int32)
    want = _merge_loop(scores, valid, 1000, carried_v, carried_i)
    got = ko.argmax_merge_ref(scores, valid, 1000, carried_v, carried_i)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    if kind == "zeros":
        np.testing.assert_array_equal(got[0], carried_v)
        np.testing.assert_array_equal(got[1], carried_i)
    if nc >= 9 and kind in ("none", "ones"):
        assert (scores == scores.max(axis=1, keepdims=True)).sum(axis=1).max() > 1   # ties do occur


def test_argmax_inputs_tie_within_and_across_lanes():
    s = ko.argmax_scores(4, 1024, seed=5)
    top = s == s.max(axis=1, keepdims=True)
    cols = [np.nonzero(t)[0] for t in top]
    for c in cols:
        lanes4 = (c // 4) % 64        # the vectorised path's lane
        lanes1 = c % 64               # the scalar path's lane
        assert len(set(lanes4)) > 1 and len(set(lanes1)) > 1
        assert len(c) > len(set(lanes4)) and len(c) > len(set(lanes1))   # two maxima in one lane
    assert ko.VALID_OFFSET % 4 != 0
    buf = ko.argmax_valid("random", 257, seed=2)
    assert 0 < buf[ko.VALID_OFFSET:ko.VALID_OFFSET + 257].sum() < 257


# ---- scan -----------------------------------------------------------------

def test_first_end_ref_is_the_first_match_end_of_scan_reference():
    tables = dfa.compile_patterns(ko.SCAN_PATTERNS, case_insensitive=False)
    rows = ko.scan_corpus()
    seen = set()
    for row in rows[:120] + rows[-5:]:
        ends = dfa.scan_reference(tables, row)
        want = ends[0][0] if ends else -1
        assert ko.first_end_ref(tables, row) == want
        seen.add(want > 0)
    assert seen == {True, False}
    assert ko.first_end_ref(tables, b"a 123-45-6789 z") == 13


def test_scan32_rows_hit_bits_0_and_31():
    for length in (6, 40):
        words = ko.literal_words_32(length, seed=21)
        tables = dfa.compile_literals(words, True)
        rows = ko.scan32_rows(words, 40, seed=4, long_row=2000)
        masks = [dfa.match_mask_reference(tables, r) for r in rows]
        assert masks[0] == 1 and masks[1] == 1 << 31 and masks[2] == (1 << 31) | 1 and masks[3] == 0
        assert masks[5] == 1 << 31 and masks[4] == 0
        assert masks[7] == (1 << 31) | 1 and len(rows[7]) == 2000
        assert ko.first_end_ref(tables, rows[7]) == 2000 - length - 1
        assert any(b >= 0x80 for r in rows for b in r)
    blob, beg, end = ko.gapped_spans(rows, b"forbidden " + words[0].encode(), first_begin=13)
    assert beg[0] == 13 and all(beg[1:] > end[:-1]) and all(blob[b:e] == r for b, e, r in zip(beg, end, rows))


# ---- featurize ------------------------------------------------------------

def test_featurize_case_shape():
    blob, beg, end = ko.featurize_case()
    lens = (end - beg).tolist()
    assert lens[:len(ko.FEATURIZE_LENGTHS)] == ko.FEATURIZE_LENGTHS
    assert beg[0] > 0 and 0 <= beg.min() and end.max() <= len(blob) and (end >= beg).all()
    assert any(b1 > e0 for e0, b1 in zip(end[:-1], beg[1:]))          # gaps
    assert any(b1 < e0 for e0, b1 in zip(end[:-1], beg[1:]))          # an overlap
    touching = [i for i in range(len(beg) - 1) if beg[i + 1] == end[i]]
    assert touching and all(chr(blob[end[i] - 1]).isalnum() and chr(blob[end[i]]).isalnum() for i in touching)
    # threads own chunks of ceil(len / 256) bytes: tokens start on a chunk's first byte
    word = lambda b: chr(b).isalnum() and b < 0x80 or b == 0x5F  # noqa: E731
    for i in (4, 6, 7, 8):   # lengths 257, 513, 4099, 20000
        span = blob[beg[i]:end[i]]
        chunk = -(-len(span) // 256)
        assert chunk > 1
        starts = [p for p in range(chunk, len(span), chunk) if word(span[p]) and not word(span[p - 1])]
        assert len(starts) >= 3


@pytest.mark.parametrize("dim", ko.FEATURIZE_DIMS)
def test_featurize_counts_are_recoverable_from_f32(dim):
    """rint(out * ||counts||) recovers the counts only if the fp32 tolerance
    times the norm stays below one half."""
    counts = ko.featurize_counts(dim)
    norms = np.sqrt((counts.astype(np.float64) ** 2).sum(axis=1))
    assert ko.FEATURIZE_ATOL * norms.max() < 0.5
    assert counts.max() >= 2 and (counts.sum(axis=1) == 0).sum() >= 2   # empty span, delimiters only
    blob, beg, end = ko.featurize_case()
    ref = featurize_batch([blob[b:e] for b, e in zip(beg, end)], dim)
    nz = norms > 0
    np.testing.assert_array_equal(np.rint(ref[nz].astype(np.float64) * norms[nz, None]).astype(np.int64), counts[nz])
    # the case duplicates land in one bucket, the 3000-byte token counts once
    n = len(ko.FEATURIZE_LENGTHS)
    assert counts[n].sum() == 1 and counts[n + 1].sum() == 0 and counts[n + 3].max() >= 4

"""Decoding against a candidate bank on the MI355X (speech_decoding_amd/retrieval.py, csrc/retrieval.hip).

Yardstick: the reference Classifier's similarity (models.py:223-232, restated as oracle.brain_oracle.topk_accuracy restates it)
in float64 on the CPU, over the operands rounded to the compute dtype: cos = <q, c> / max(|q| |c|, 1e-8).  Neighbouring top-k
scores of these inputs are often closer than 1e-5, so nothing here compares index lists row by row; every check is
tie-tolerant by construction and no row is skipped.  TOL = 1e-4 is the project's exact-path tolerance; the 16-bit paths
multiply exactly into fp32 accumulators, so it serves them too on same-rounded operands.

Measured on the MI355X, max |score - fp64 score| over all cases of a dtype: fp32 2.7e-7, bf16 1.3e-7, fp16 1.2e-7 (MEASURED below);
the selection kernel on its own scores: equal to the CPU's fp32 result in every bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O      # noqa: E402,F401  (the yardstick's formula: topk_accuracy)
from tests import builders as TB          # noqa: E402

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
TOL = 1e-4
SHAPES = {"a": (96, 1000, 64, 90), "b": (40, 300, 24, 50)}
SMALL_SCRATCH = 64 << 10      # (96, 1000, 64, 90): 8 query rows per block, 256 bank rows per chunk (test_retrieval_cpu.py)
# largest |score - fp64 score| seen on the MI355X, all cases of the dtype (the checks below use TOL, not these)
MEASURED = {"fp32": 2.7e-7, "bf16": 1.3e-7, "fp16": 1.2e-7}

_cases = {}


def case(shape: str, dtype: str):
    """Seeded inputs of one (shape, dtype) and their fp64 cosine matrix, computed once and shared (never written to)."""
    key = (shape, dtype)
    if key not in _cases:
        N, M, F, T = SHAPES[shape]
        g = torch.Generator().manual_seed(1234 + 17 * N + M)
        bank = torch.randn(M, F, T, generator=g)
        labels = torch.randint(M, (N,), generator=g)
        queries = 0.35 * bank[labels] + torch.randn(N, F, T, generator=g)
        _cases[key] = (queries, bank, labels, cosine64(queries, bank, dtype))
    return _cases[key]


def cosine64(queries, bank, dtype):
    q = queries.to(DT[dtype]).double().reshape(queries.shape[0], -1)
    c = bank.to(DT[dtype]).double().reshape(bank.shape[0], -1)
    den = torch.clamp(q.norm(dim=-1)[:, None] * c.norm(dim=-1)[None, :], min=1e-8)
    return (q @ c.T) / den


def check_against_fp64(res, ref, labels, k, what=""):
    """Checks 1-4 of the module docstring's yardstick; returns the largest score error."""
    N, M = ref.shape
    idx, sc = res.indices.cpu(), res.scores.cpu().double()
    assert idx.shape == (N, k) and idx.dtype == torch.int64 and res.scores.dtype == torch.float32
    top = torch.sort(ref, dim=1, descending=True).values[:, :k]
    err1 = float((sc - top).abs().max())
    assert idx.min() >= 0 and idx.max() < M
    assert all(len(set(row.tolist())) == k for row in idx), "indices repeat within a row"
    err2 = float((torch.gather(ref, 1, idx) - sc).abs().max())
    print(f"{what}: max |score - r-th largest fp64| {err1:.3e}, max |score - fp64 score of its index| {err2:.3e}")
    assert err1 <= TOL and err2 <= TOL
    s32 = res.scores.cpu()
    assert bool((s32[:, 1:] <= s32[:, :-1]).all()), "scores are not non-increasing"
    tied = s32[:, 1:] == s32[:, :-1]
    assert bool((idx[:, 1:] > idx[:, :-1])[tied].all()), "equal scores not in ascending index order"
    if labels is not None:
        check_ranks(res.ranks, ref, labels)
    return max(err1, err2)


def check_ranks(ranks, ref, labels):
    """#{j : s_j > s_l + 2 TOL} <= rank <= #{j != l : s_j >= s_l - 2 TOL} in fp64."""
    N, M = ref.shape
    r = ranks.cpu()
    assert r.dtype == torch.int32 and r.shape == (N,)
    sl = ref[torch.arange(N), labels][:, None]
    lo = (ref > sl + 2 * TOL).sum(dim=1)
    other = torch.arange(M)[None, :] != labels[:, None]
    hi = ((ref >= sl - 2 * TOL) & other).sum(dim=1)
    assert bool((lo <= r).all()) and bool((r <= hi).all()), (lo.tolist(), r.tolist(), hi.tolist())


def run(shape, dtype, k=10, with_labels=True, **kw):
    from speech_decoding_amd import SpeechBank, retrieve
    queries, bank, labels, ref = case(shape, dtype)
    b = SpeechBank.from_tensor(bank.to(DEV), dtype=DT[dtype])
    res = retrieve(queries.to(DEV), b, k=k, labels=labels.to(DEV) if with_labels else None, **kw)
    return res, ref, labels


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_topk_scores_indices_order_and_ranks(shape, dtype):
    res, ref, labels = run(shape, dtype)
    assert res.indices.is_cuda and res.scores.is_cuda and res.ranks.is_cuda
    check_against_fp64(res, ref, labels, 10, f"{SHAPES[shape]} {dtype}")
    # the planted candidates: the fp64 yardstick itself puts every one of them first
    assert bool((ref.argmax(dim=1) == labels).all())
    assert res.accuracy(1) == res.accuracy(10) == 1.0


def test_k_64():
    res, ref, labels = run("a", "bf16", k=64)
    check_against_fp64(res, ref, labels, 64, "k = 64")


def test_without_labels_there_are_no_ranks():
    res, ref, _ = run("b", "fp32", with_labels=False)
    assert res.ranks is None
    check_against_fp64(res, ref, None, 10, "no labels")
    with pytest.raises(ValueError):
        res.accuracy(1)


def test_host_labels_and_device_labels_agree():
    from speech_decoding_amd import SpeechBank, retrieve
    queries, bank, labels, _ = case("b", "bf16")
    b = SpeechBank.from_tensor(bank.to(DEV))
    on_dev = retrieve(queries.to(DEV), b, labels=labels.to(DEV))
    for host in (labels, labels.tolist(), labels.numpy().astype(np.int32)):
        assert torch.equal(retrieve(queries.to(DEV), b, labels=host).ranks, on_dev.ranks)
    outside = labels.clone()
    outside[3] = len(b)
    with pytest.raises(IndexError):
        retrieve(queries.to(DEV), b, labels=outside)
    r = retrieve(queries.to(DEV), b, labels=outside.to(DEV)).ranks       # device labels: nothing is read back, the kernel flags it
    assert int(r[3]) == -1 and torch.equal(r[:3], on_dev.ranks[:3]) and torch.equal(r[4:], on_dev.ranks[4:])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the selection kernel alone, to the bit
# ---------------------------------------------------------------------------------------------------------------------------
def expected_selection(S, qsq, csq, labels, k):
    """CPU fp32: the kernel's formula, a stable sort by (-score, index), a plain count for the ranks."""
    den = torch.clamp(torch.sqrt(qsq)[:, None] * torch.sqrt(csq)[None, :], min=1e-8)
    s = S / den + 0.0                                   # (-0 -> +0)
    order = torch.sort(-s, dim=1, stable=True).indices[:, :k]
    n, M = S.shape
    sl = s[torch.arange(n), labels][:, None]
    j = torch.arange(M)[None, :]
    ranks = ((s > sl) | ((s == sl) & (j < labels[:, None]))).sum(dim=1).to(torch.int32)
    return order, torch.gather(s, 1, order), ranks


def chunk_major(S, chunk_cols):
    """The layout one GEMM per bank chunk leaves: chunk c = [n][pad64(its columns)]; padding columns hold NaN here."""
    n, M = S.shape
    parts = []
    for c0 in range(0, M, chunk_cols):
        m = min(chunk_cols, M - c0)
        blk = torch.full((n, (m + 63) // 64 * 64), float("nan"))
        blk[:, :m] = S[:, c0: c0 + m]
        parts.append(blk.reshape(-1))
    return torch.cat(parts)


def selection_matrix(n, M, seed):
    """Exactly repeated values on purpose: few distinct integers, duplicate columns, a zero column, a zero-norm row, a constant
    row, and rows that rise / fall along the bank (a rising row improves its top-k at every step of the kernel)."""
    g = torch.Generator().manual_seed(seed)
    S = torch.randint(-40, 41, (n, M), generator=g).float()
    csq = torch.randint(1, 5, (M,), generator=g).float() * 16.0
    qsq = torch.randint(1, 4, (n,), generator=g).float()
    if M > 8:
        S[:, 5] = S[:, 2]; csq[5] = csq[2]                       # duplicate columns
        S[:, M - 1] = S[:, 2]; csq[M - 1] = csq[2]
        S[:, 7] = 0.0; csq[7] = 0.0                              # a zero column (zero candidate)
    if n > 4:
        S[0] = 0.0; qsq[0] = 0.0                                 # a zero-norm query: every score 0, order = index order
        S[1] = 3.0                                               # a constant row of dots
        S[2] = torch.arange(M).float(); S[3] = -torch.arange(M).float()
        S[4] = (torch.arange(M) // 7).float()                    # rising in plateaus
    labels = torch.randint(M, (n,), generator=g)
    if n > 4 and M > 8:
        labels[0], labels[1], labels[2] = M // 2, 5, M - 1
    return S, qsq, csq, labels


@pytest.mark.parametrize("n,M,k,chunk", [(7, 9001, 64, None), (7, 9001, 10, 2048), (6, 20000, 64, 8192), (5, 4096, 64, None),
                                         (5, 4097, 33, 256), (3, 70, 64, None), (3, 64, 64, None), (2, 1, 1, None), (5, 300, 10, 128)])
def test_selection_kernel_is_exact_on_its_own_scores(n, M, k, chunk):
    from speech_decoding_amd import ops
    S, qsq, csq, labels = selection_matrix(n, M, seed=n * 100003 + M)
    want_idx, want_sc, want_rank = expected_selection(S, qsq, csq, labels, k)
    layout = chunk_major(S, chunk if chunk is not None else (M + 63) // 64 * 64)
    idx, sc, rank = ops.retrieval_select(layout.to(DEV), qsq.to(DEV), csq.to(DEV), n, M, k, chunk, labels=labels.to(DEV))
    assert torch.equal(idx.cpu(), want_idx)
    assert torch.equal(sc.cpu().view(torch.int32), want_sc.view(torch.int32))          # bits, not values
    assert torch.equal(rank.cpu(), want_rank)
    idx2, sc2, none = ops.retrieval_select(layout.to(DEV), qsq.to(DEV), csq.to(DEV), n, M, k, chunk)
    assert none is None and torch.equal(idx2, idx) and torch.equal(sc2, sc)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. blocking
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_small_scratch_forces_blocks_and_chunks_and_still_passes(dtype):
    from speech_decoding_amd.retrieval import plan_blocks
    from speech_decoding_amd import lib as L
    N, M, F, T = SHAPES["a"]
    nb, mc, _, _ = plan_blocks(N, M, L.rows_tp(T) * L.pad_channels(F), DT[dtype], SMALL_SCRATCH)
    assert nb < N and mc < M
    res, ref, labels = run("a", dtype, scratch_bytes=SMALL_SCRATCH)
    check_against_fp64(res, ref, labels, 10, f"small scratch {dtype}")
    assert res.accuracy(1) == 1.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_single_query(dtype):
    from speech_decoding_amd import SpeechBank, retrieve
    queries, bank, labels, ref = case("a", dtype)
    b = SpeechBank.from_tensor(bank.to(DEV), dtype=DT[dtype])
    res = retrieve(queries[5:6].to(DEV), b, k=10, labels=labels[5:6])
    check_against_fp64(res, ref[5:6], labels[5:6], 10, f"N = 1 {dtype}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_bank_built_in_uneven_adds_equals_bank_built_at_once(dtype):
    from speech_decoding_amd import SpeechBank, retrieve
    queries, bank, labels, _ = case("a", dtype)
    whole = SpeechBank.from_tensor(bank.to(DEV), dtype=DT[dtype])
    parts = SpeechBank(bank.shape[1], bank.shape[2], dtype=DT[dtype], device=DEV)        # grows as needed
    got = [parts.add(bank[a:b].to(DEV)) for a, b in ((0, 1), (1, 613), (613, 1000))]
    assert got == [range(0, 1), range(1, 613), range(613, 1000)] and len(parts) == len(whole) == 1000
    assert parts.rows.dtype == DT[dtype] and parts.rows.shape == whole.rows.shape
    assert torch.equal(parts.rows.view(torch.uint8), whole.rows.view(torch.uint8))
    assert torch.equal(parts.norms_sq.view(torch.int32), whole.norms_sq.view(torch.int32))
    for scratch in (SMALL_SCRATCH, 1 << 30):
        a = retrieve(queries.to(DEV), whole, labels=labels, scratch_bytes=scratch)
        b = retrieve(queries.to(DEV), parts, labels=labels, scratch_bytes=scratch)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. determinism, and no interference with the loss's caches and rings
# ---------------------------------------------------------------------------------------------------------------------------
def test_same_call_same_bits_also_around_a_clip_loss_step():
    from speech_decoding_amd import SpeechBank, retrieve
    queries, bank, labels, _ = case("a", "bf16")
    b = SpeechBank.from_tensor(bank.to(DEV))
    q = queries.to(DEV)
    first = retrieve(q, b, labels=labels)
    second = retrieve(q, b, labels=labels)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    g = torch.Generator().manual_seed(7)
    lossf = TB.clip_loss(5.1, DEV)
    Y = torch.randn(12, 64, 90, generator=g).to(DEV)
    Z = torch.randn(12, 64, 90, generator=g).to(DEV).requires_grad_(True)
    loss1 = lossf(Y, Z)
    loss1.backward()
    third = retrieve(q, b, labels=labels)
    assert all(torch.equal(x, y) for x, y in zip(first, third))
    Z2 = Z.detach().clone().requires_grad_(True)
    loss2 = lossf(Y, Z2)                                  # and the loss is not disturbed by the retrieval in between
    loss2.backward()
    assert torch.equal(loss1.detach(), loss2.detach()) and torch.equal(Z.grad, Z2.grad)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the square case against the existing Classifier, and Classifier.decode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_square_case_agrees_with_classifier_ranks(dtype):
    from speech_decoding_amd import SpeechBank, retrieve
    from speech_decoding.models import Classifier
    B, F, T = 96, 64, 90
    g = torch.Generator().manual_seed(99)
    Z = torch.randn(B, F, T, generator=g)
    Y = 0.2 * Z + torch.randn(B, F, T, generator=g)
    ref = cosine64(Y, Z, dtype)                          # rows: speech, columns: brain — both calls look this way
    diag = torch.arange(B)
    Zd, Yd = Z.to(DT[dtype]).to(DEV), Y.to(DEV)
    res = retrieve(Yd, SpeechBank.from_tensor(Zd, dtype=DT[dtype]), labels=diag)
    check_ranks(res.ranks, ref, diag)
    clf = Classifier(TB.Config())
    check_ranks(clf.ranks(Zd, Yd), ref, diag)
    # Classifier.decode: brain queries against a speech bank = retrieve the other way round
    bank = SpeechBank.from_tensor(Yd, dtype=DT[dtype])
    a = clf.decode(Zd, bank, k=7, labels=diag)
    b = retrieve(Zd, bank, k=7, labels=diag)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    check_against_fp64(a, cosine64(Z, Y, dtype), diag, 7, f"decode {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the encoder's zero-copy output as queries
# ---------------------------------------------------------------------------------------------------------------------------
def test_encoder_output_view_equals_its_contiguous_copy():
    from speech_decoding_amd import SpeechBank, retrieve
    from speech_decoding_amd import ops
    d, B = dict(TB.TOY, T=90), 12
    F, T = d["F"], d["T"]
    _, P, X, Y, subj = TB.toy_problem(d, B)
    enc = TB.build_encoder(P, d, DEV, training=False)
    with torch.no_grad():
        Z = enc(X.to(DEV), subj)
    assert not Z.is_contiguous() and ops.rows_base(Z, B, F, T, torch.float32) is not None       # the zero-copy rows view
    bank = SpeechBank.from_tensor(Y.to(DEV), dtype=torch.float32)
    labels = torch.arange(B)
    a = retrieve(Z, bank, k=5, labels=labels)
    b = retrieve(Z.contiguous(), bank, k=5, labels=labels)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    check_against_fp64(a, cosine64(Z.cpu(), Y, "fp32"), labels, 5, "encoder view")
    # and the view goes into a bank without a copy of its own being needed
    zb = SpeechBank.from_tensor(Z, dtype=torch.float32)
    zc = SpeechBank.from_tensor(Z.contiguous(), dtype=torch.float32)
    assert torch.equal(zb.rows, zc.rows) and torch.equal(zb.norms_sq, zc.norms_sq)

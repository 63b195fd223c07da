"""GPU: the gather / scatter / reorder kernels of the train backward, one at a time, against plain torch on the CPU in int64 / fp64:
the fp32 GEMM's row maps and its split-K reduce (gemm.hip), embedding_grad, colsum, gather_rows and transpose (misc.hip),
split_planes_dual with a row map, all three outputs and the fused CE-gradient transform (split.hip).

Inputs are small integers stored as fp32 unless a case says otherwise: every partial sum stays far below 2^24, so any summation
order is exact and the assertion is torch.equal - a difference is a wrong index, a dropped tail or a double count, never rounding.
The plane images are compared bitwise with ops.split_planes of a materialised input (that layout is pinned by the GEMM tests)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ints(*shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _r(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _stored(n, inner, outer):
    """stored row of logical row r under the row map (inner, outer) - common.h: (r % inner) * outer + r / inner"""
    r = torch.arange(n)
    return (r % inner) * outer + r // inner


def _idx(n, V, seed):
    """n ids in [0, V) with duplicates that include both ends"""
    idx = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))
    idx[0], idx[1], idx[n - 1], idx[n // 2] = V - 1, 0, 0, V - 1
    return idx


# ------------------------------------------------------------------------------------------------ mapped fp32 GEMM, no split
@pytest.mark.parametrize("K,ld", [(40, 40), (41, 41), (40, 72)])
def test_gemm_gather_on_a(lib, K, ld):
    """C = table[idx] · B^T: the embedding lookup as the GEMM's own A rows.  ld = 40 / 72: 16-byte loads (72: the table is the left
    column block of a wider tensor, as word_w_ih's blocks are read); K = ld = 41: the scalar path.  300 rows: three row tiles."""
    from s2vt_video_caption_amd import ops
    V, N = 50, 130
    wide = _ints(V, ld, seed=1)
    table = wide[:, :K]
    b = _ints(N, K, seed=2)
    idx = _idx(300, V, seed=3)
    ref = (table[idx].double() @ b.double().t()).float()
    out = torch.full((300, N), 0.5, device=DEV)
    ops.gemm_mapped(wide.to(DEV)[:, :K], b.to(DEV), out, amap=idx.int().to(DEV))
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("K", [40, 33])
@pytest.mark.parametrize("inner,outer", [(37, 5), (5, 37)])
def test_gemm_perm_on_c(lib, inner, outer, K):
    """cmap = perm(L, B) (feat_proj: batch-major rows land time-major) and perm(B, L - 1) (logits: time-major rows land
    batch-major) at (B, L) = (5, 37): M = 185 is two row tiles, the second ragged.  With bias, and accumulating into a prefilled
    C; C is a column block of a wider tensor whose other columns must stay as they were."""
    from s2vt_video_caption_amd import ops
    M, N, PADC = 185, 130, 5
    a, b, bias = _ints(M, K, seed=4), _ints(N, K, seed=5), _ints(N, seed=6)
    full = (a.double() @ b.double().t()).float()
    s = _stored(M, inner, outer)
    assert sorted(s.tolist()) == list(range(M))
    c0 = _ints(M, N, seed=7)
    for use_bias, acc in ((True, False), (False, True), (True, True), (False, False)):
        want = c0.clone() if acc else torch.zeros(M, N)
        want[s] += full + (bias if use_bias else 0.0)
        buf = torch.full((M, N + PADC), -999.5)
        buf[:, :N] = c0
        buf = buf.to(DEV)
        ops.gemm_mapped(a.to(DEV), b.to(DEV), buf[:, :N], cmap=(inner, outer), bias=bias.to(DEV) if use_bias else None, accumulate=acc)
        got = buf.cpu()
        assert torch.equal(got[:, :N], want), (use_bias, acc)
        assert (got[:, N:] == -999.5).all(), "columns beyond N were written"


@pytest.mark.parametrize("M,N", [(152, 92), (150, 93)])
def test_gemm_perm_on_k_rows(lib, M, N):
    """The weight-gradient forms of the fp32 backward, C = A^T B over K = 7 * 41 = 287 stored rows (the k loop ends mid-tile):
    out_w's (perm(L - 1, B) on the k rows of B: dlogits rows are batch-major, the hidden states time-major), feat_w's
    (perm(B, L)), and the same maps on the k rows of A^T.  (152, 92): 16-byte loads; (150, 93): the scalar path."""
    from s2vt_video_caption_amd import ops
    K = 287
    at, bt = _ints(K, M, seed=8), _ints(K, N, seed=9)          # both stored as rows of k
    for inner, outer in ((41, 7), (7, 41)):
        s = _stored(K, inner, outer)
        for on_a, on_b in ((False, True), (True, False), (True, True)):
            al = at[s] if on_a else at
            bl = bt[s] if on_b else bt
            ref = (al.double().t() @ bl.double()).float()
            out = torch.full((M, N), 0.5, device=DEV)
            ops.gemm_mapped(at.to(DEV), bt.to(DEV), out, a_kmajor=False, b_kmajor=False, amap=(inner, outer) if on_a else None,
                            bmap=(inner, outer) if on_b else None)
            assert torch.equal(out.cpu(), ref), (inner, outer, on_a, on_b)
    # A[M,K] · B[K,N] with the permutation on B's k rows (the data-gradient layout)
    a = _ints(M, K, seed=10)
    s = _stored(K, 41, 7)
    out = torch.full((M, N), 0.5, device=DEV)
    ops.gemm_mapped(a.to(DEV), bt.to(DEV), out, b_kmajor=False, bmap=(41, 7))
    assert torch.equal(out.cpu(), (a.double() @ bt[s].double()).float())


def test_gemm_refuses_a_gather_on_k_rows(lib):
    from s2vt_video_caption_amd import capi, ops
    at, bt = _ints(16, 8, seed=1).to(DEV), _ints(16, 8, seed=2).to(DEV)
    out = torch.zeros(8, 8, device=DEV)
    idx = torch.arange(16, dtype=torch.int32, device=DEV)
    for kw in (dict(a_kmajor=False, b_kmajor=False, amap=idx), dict(a_kmajor=False, b_kmajor=False, bmap=idx)):
        with pytest.raises(capi.S2VTHipError, match="a gather index is only supported on operands whose stored rows are m / n"):
            ops.gemm_mapped(at, bt, out, **kw)


# ------------------------------------------------------------------------------------------------ mapped fp32 GEMM, split-K
SK_K = 1024


@functools.lru_cache(maxsize=None)
def _splitk_problem():
    """A [513, K], B [1001, K], bias, C0 and A·B^T once for every split-K case (sub-blocks of it are the smaller shapes)"""
    a, b = _ints(513, SK_K, seed=11), _ints(1001, SK_K, seed=12)
    return dict(a=a.to(DEV), b=b.to(DEV), bias=_ints(1001, seed=13).to(DEV), c0=_ints(513, 1001, seed=14).to(DEV),
                full=(a.double() @ b.double().t()).float().to(DEV))


def _slabs_written(ws, MN, sentinel):
    """number of leading M*N slabs of the scratch that hold no sentinel any more; everything behind them must be untouched"""
    n = 0
    while (n + 1) * MN <= ws.numel() and not bool((ws[n * MN:(n + 1) * MN] == sentinel).any()):
        n += 1
    assert bool((ws[n * MN:] == sentinel).all()), "a slab was written in part, or the scratch was written past the last slab"
    return n


# 513 x 1000 / 1001 is 40 tiles: the launcher's plan stops at 6 slices there (a 7th would start a second round of the 256 compute
# units); 385 x 1000 / 1001 is 32 tiles, where it goes on to 8.  The cap holds it at 2, 3 and 5.
@pytest.mark.parametrize("N", [1000, 1001])
@pytest.mark.parametrize("M,cap,slabs", [(513, 2, 2), (513, 3, 3), (513, 5, 5), (513, 0, 6), (385, 8, 8)])
def test_gemm_splitk_every_reduce_variant(lib, M, cap, slabs, N):
    """splitk_reduce_kernel: slab counts 2, 3, 5, 6, 8 (its loop takes four at a time: every tail length) x bias x accumulate x C
    contiguous (16-byte stores) / a column block of a wider tensor with an odd row stride (scalar stores) / cmap = perm.  N = 1001
    runs the scalar reduce.  The scratch is pre-filled with 0.5, which no integer result equals: the count of overwritten slabs
    proves that the split ran, with exactly `slabs` slices."""
    from s2vt_video_caption_amd import ops
    p = _splitk_problem()
    a, b, bias = p["a"][:M], p["b"][:N], p["bias"][:N]
    full, c0 = p["full"][:M, :N], p["c0"][:M, :N]
    MN = M * N
    inner, outer = (19, 27) if M == 513 else (35, 11)
    s = _stored(M, inner, outer).to(DEV)
    for layout in ("contiguous", "odd_ld", "perm"):
        for use_bias in (False, True):
            for acc in (False, True):
                want = c0.clone() if acc else torch.zeros(M, N, device=DEV)
                upd = full + bias if use_bias else full
                if layout == "perm":
                    want[s] += upd
                else:
                    want += upd
                buf = torch.full((M, N + 1 + N % 2), -999.5, device=DEV)        # an odd row stride
                out = buf[:, :N] if layout == "odd_ld" else torch.empty(M, N, device=DEV)
                out.copy_(c0)
                ws = torch.full((9 * MN + 16,), 0.5, device=DEV)
                ops.gemm_mapped(a, b, out, cmap=(inner, outer) if layout == "perm" else None, bias=bias if use_bias else None,
                                accumulate=acc, splitk_ws=ws, splitk_cap=cap)
                assert _slabs_written(ws, MN, 0.5) == slabs, (layout, use_bias, acc)
                assert torch.equal(out, want), (layout, use_bias, acc)
                if layout == "odd_ld":
                    assert buf.stride(0) % 2 == 1 and bool((buf[:, N:] == -999.5).all())


@pytest.mark.parametrize("M,N,cap,slabs", [(512, 1000, 0, 8), (513, 1001, 5, 5)])
def test_gemm_splitk_of_k_row_operands_with_perm(lib, M, N, cap, slabs):
    """The weight-gradient form under split-K, as the fp32 backward runs it (feat_w: K = L * B rows, few tiles): A^T and B stored
    as rows of k, both read through perm(16, 64), every slice a range of those permuted rows.  (512, 1000): 16-byte loads."""
    from s2vt_video_caption_amd import ops
    p = _splitk_problem()
    s = _stored(SK_K, 16, 64).to(DEV)
    at, bt = torch.empty(SK_K, M, device=DEV), torch.empty(SK_K, N, device=DEV)
    at[s], bt[s] = p["a"][:M].t(), p["b"][:N].t()                    # logical k row = stored row s[k]
    out = torch.full((M, N), 0.5, device=DEV)
    ws = torch.full((9 * M * N + 16,), 0.5, device=DEV)
    ops.gemm_mapped(at, bt, out, a_kmajor=False, b_kmajor=False, amap=(16, 64), bmap=(16, 64), splitk_ws=ws, splitk_cap=cap)
    assert _slabs_written(ws, M * N, 0.5) == slabs
    assert torch.equal(out, p["full"][:M, :N])


def test_gemm_splitk_random_data_is_deterministic(lib):
    """Random fp32 operands through five slices against fp64, at the bound of test_gemm_all_layouts (fp32 accumulation over K
    terms of O(1) products), and two runs bit for bit the same (the slices are summed in a fixed order)."""
    from s2vt_video_caption_amd import ops
    M, N, K = 513, 1000, SK_K
    a, b, bias = _r(M, K, seed=15), _r(N, K, seed=16), _r(N, seed=17)
    ref = a.double() @ b.double().t() + bias.double()
    tol = 2e-6 * K ** 0.5 * 4 + 1e-6
    ad, bd, biasd = a.to(DEV), b.to(DEV), bias.to(DEV)
    outs = []
    for _ in range(2):
        ws = torch.full((9 * M * N + 16,), 1e30, device=DEV)
        out = torch.empty(M, N, device=DEV)
        ops.gemm_mapped(ad, bd, out, bias=biasd, splitk_ws=ws, splitk_cap=5)
        assert _slabs_written(ws, M * N, 1e30) == 5
        outs.append(out.cpu())
    err = (outs[0].double() - ref).abs().max().item()
    print("split-K (5 slices) max |err| vs fp64 = %.3e, bound %.3e" % (err, tol))
    assert err < tol
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ embedding_grad
EG_CAP = 64          # misc.hip: a token with more matches than this is summed by the heavy kernel


def _token_list(rows, V, seed, top=700, more=(100, 130, 200, 300, 400, 500), light=41):
    """Every path of embedding_grad in one list: token 0 never occurs; tokens with 1, 63, 64, 65, 66 and 700 occurrences; six more
    heavy ones (with token V - 1 ten in all: more than the heavy kernel's gridDim.y = 4); light ones with 2..42; token V - 1
    takes the rest (> 8192 + 1024 of 20037 rows: its matches straddle the heavy kernel's pass boundary and go on into the last,
    partial block of 1024 rows).  Shuffled."""
    counts = [0, 1, 63, 64, 65, 66, top] + list(more)
    counts += [(3 * i) % light + 2 for i in range(len(counts), V - 1)]
    assert len(counts) == V - 1 and sum(counts) < rows
    counts.append(rows - sum(counts))
    tok = torch.repeat_interleave(torch.arange(V), torch.tensor(counts))
    return tok[torch.randperm(rows, generator=torch.Generator().manual_seed(seed))], torch.tensor(counts)


def _embedding_grad_checked(ops, lib, d, tok, V):
    """run the kernel on NaN-poisoned d_emb and garbage scratch; returns d_emb (CPU) after checking what the call leaves in its
    scratch: the per-token counts (the wave-aggregated count kernel) and the list of heavy tokens (those with > EG_CAP matches)"""
    rows, E = d.shape
    n_ws = lib.s2vt_embedding_grad_ws_ints(rows, V)
    ws = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_ws,), generator=torch.Generator().manual_seed(rows + E)).int().to(DEV)
    out = torch.full((V, E), float("nan"), device=DEV)
    ops.embedding_grad(d.to(DEV), tok.int().to(DEV), V, out=out, ws=ws)
    w = ws.cpu().long()
    max_heavy = rows // EG_CAP + 2
    counts = torch.bincount(tok, minlength=V)
    assert torch.equal(w[max_heavy + 1:], counts)
    heavy = torch.nonzero(counts > EG_CAP).flatten()
    assert int(w[max_heavy]) == heavy.numel()
    assert sorted(w[:heavy.numel()].tolist()) == heavy.tolist()
    return out.cpu()


def _index_add_exact(d, tok, V):
    return torch.zeros(V, d.shape[1], dtype=torch.int64).index_add_(0, tok, d.long()).float()


@pytest.mark.parametrize("E", [24, 1])
def test_embedding_grad_every_path_in_one_list(lib, E):
    """rows = 20037 (no multiple of 256 or 1024), V = 50; E = 24 leaves the heavy kernel a partial second block of 16 columns."""
    from s2vt_video_caption_amd import ops
    rows, V = 20000 + 37, 50
    tok, counts = _token_list(rows, V, seed=21)
    assert int(counts[V - 1]) > 8192 + 1024 and int((counts > EG_CAP).sum()) >= 9
    last_block = tok[rows // 1024 * 1024:]
    assert 0 < last_block.numel() < 1024 and bool((last_block == V - 1).any())
    assert int((tok[:9 * 1024] == V - 1).sum()) <= 8192 < int((tok[:11 * 1024] == V - 1).sum())      # the first pass ends inside
    d = _ints(rows, E, seed=22)
    assert torch.equal(_embedding_grad_checked(ops, lib, d, tok, V), _index_add_exact(d, tok, V))


@pytest.mark.parametrize("E", [300, 1])
def test_embedding_grad_short_list(lib, E):
    """A 3000-row list at E = 300 (the light kernel's column loop of 256 threads takes a second round) and E = 1; ids 0 and V - 1
    both occur."""
    from s2vt_video_caption_amd import ops
    rows, V = 3000, 50
    tok, counts = _token_list(rows, V, seed=23, top=300, more=(100, 130), light=7)
    assert int(counts[V - 1]) > 1024
    tok = (tok + 1) % V                                   # token 0 takes the large count, token 1 none
    d = _ints(rows, E, seed=24)
    assert torch.equal(_embedding_grad_checked(ops, lib, d, tok, V), _index_add_exact(d, tok, V))


@pytest.mark.parametrize("rows", [20037, 0])
def test_embedding_grad_one_token_and_no_rows(lib, rows):
    """every row the same token (three passes of the heavy kernel, the last partial); rows = 0: all of d_emb is written as zeros"""
    from s2vt_video_caption_amd import ops
    V, E = 50, 24
    tok = torch.full((rows,), 17, dtype=torch.long)
    d = _ints(rows, E, seed=25)
    got = _embedding_grad_checked(ops, lib, d, tok, V)
    assert torch.equal(got, _index_add_exact(d, tok, V))
    if rows == 0:
        assert torch.equal(got, torch.zeros(V, E))


def test_embedding_grad_random_data_is_deterministic(lib):
    """Random fp32 rows against fp64 index_add_.  Row v is a sum of n_v fp32 terms in some fixed order: |error| <= n_v * 2^-24 *
    sum |terms| per element, whatever the order (the standard bound of an n-term floating-point sum); two runs are bitwise equal."""
    from s2vt_video_caption_amd import ops
    rows, V, E = 20037, 50, 24
    tok, counts = _token_list(rows, V, seed=26)
    d = _r(rows, E, seed=27)
    ref = torch.zeros(V, E, dtype=torch.float64).index_add_(0, tok, d.double())
    bound = counts.double()[:, None] * 2.0 ** -24 * torch.zeros(V, E, dtype=torch.float64).index_add_(0, tok, d.double().abs())
    a = _embedding_grad_checked(ops, lib, d, tok, V)
    b = _embedding_grad_checked(ops, lib, d, tok, V)
    err = (a.double() - ref).abs()
    print("embedding_grad max |err| / bound = %.3f" % (err / bound.clamp_min(1e-300)).max().item())
    assert bool((err <= bound).all())
    assert torch.equal(a, b)


def test_embedding_grad_of_a_caption_batch(lib):
    """The real token distribution: a synth.make_batch caption batch at B = 64 through ops.tokens_time_major - <pad> and <eos>
    heavy, most of the vocabulary unused."""
    from s2vt_video_caption_amd import ops, synth
    B, L, V, E = 64, 80, 12000, 24
    _, caps, _ = synth.make_batch(B, L, 8, V, seed=28)
    tok = ops.tokens_time_major(caps.to(DEV), L - 1, V).cpu().long()
    assert torch.equal(tok, caps[:, :L - 1].t().reshape(-1))
    counts = torch.bincount(tok, minlength=V)
    assert int(counts[0]) > EG_CAP and int(counts[3]) == B and int((counts == 0).sum()) > V // 2
    d = _ints(tok.numel(), E, seed=29)
    assert torch.equal(_embedding_grad_checked(ops, lib, d, tok, V), _index_add_exact(d, tok, V))


# ------------------------------------------------------------------------------------------------ split_planes_dual
def _planes_equal(ops, got, x_dev, nplanes, transpose=False):
    want, _, _ = ops.split_planes(x_dev, nplanes=nplanes, transpose=transpose)
    assert got.shape == want.shape
    return torch.equal(got, want)


def _bitwise_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _chunk_sums(x):
    """exact integer column sums of each 64-row chunk"""
    return torch.stack([x[r:r + 64].long().sum(0) for r in range(0, x.shape[0], 64)]).float()


@pytest.mark.parametrize("nplanes", [3, 1])
def test_split_dual_gather_and_perm_maps(lib, nplanes):
    from s2vt_video_caption_amd import ops
    emb = _r(50, 40, seed=31)
    idx = _idx(150, 50, seed=32)
    res = ops.split_planes_dual(emb.to(DEV), nplanes, rowmap=idx.int().to(DEV), want_t=True)
    mat = emb[idx].to(DEV)
    assert _planes_equal(ops, res["r"], mat, nplanes) and _planes_equal(ops, res["t"], mat, nplanes, transpose=True)
    x = _r(135, 70, seed=33)
    for inner, outer in ((27, 5), (5, 27)):
        res = ops.split_planes_dual(x.to(DEV), nplanes, rowmap=(inner, outer), want_t=True)
        mat = x[_stored(135, inner, outer)].to(DEV)
        assert _planes_equal(ops, res["r"], mat, nplanes) and _planes_equal(ops, res["t"], mat, nplanes, transpose=True)


@pytest.mark.parametrize("ld", [70, 71])
@pytest.mark.parametrize("nplanes", [3, 1])
def test_split_dual_all_three_outputs(lib, nplanes, ld):
    """rows = 130: three 64-row chunks, the last of 2 rows; cols = 70: two column tiles, no multiple of 4; ld = 71: a view on
    which the 16-byte loads must switch off.  Row planes, transposed planes and the chunks' column sums from ONE call."""
    from s2vt_video_caption_amd import ops
    rows, cols = 130, 70
    x = _ints(rows, cols, seed=34)
    xd = torch.full((rows, ld), 77.0, device=DEV)
    xd[:, :cols] = x.to(DEV)
    res = ops.split_planes_dual(xd[:, :cols], nplanes, want_t=True, want_colpart=True)
    mat = x.to(DEV)
    assert _planes_equal(ops, res["r"], mat, nplanes)
    assert _planes_equal(ops, res["t"], mat, nplanes, transpose=True)
    assert torch.equal(res["colpart"].cpu(), _chunk_sums(x))
    total = x.long().sum(0).float()
    assert torch.equal(ops.colsum_finish(res["colpart"]).cpu(), total)
    pre = _ints(cols, seed=35)
    assert torch.equal(ops.colsum_finish(res["colpart"], out=pre.to(DEV), accumulate=True).cpu(), pre + total)


def _ce_problem(lib, V, gout, seed):
    """logits [5 * 27, V], targets with both ends of the vocabulary, lse from s2vt_mean_ce_forward"""
    B, Lm1 = 5, 27
    R = B * Lm1
    logits = _r(R, V, seed=seed, scale=3.0).to(DEV)
    target = torch.randint(0, V, (B, Lm1 + 1), generator=torch.Generator().manual_seed(seed + 1))
    target[0, 1], target[1, 2], target[B - 1, Lm1] = 0, V - 1, V - 1
    target = target.to(DEV)
    scratch = torch.empty(2 * R + 1, device=DEV)
    lse = scratch[:R]
    from s2vt_video_caption_amd import capi
    capi.check(lib.s2vt_mean_ce_forward(B, Lm1, V, logits.data_ptr(), target.data_ptr(), target.stride(0), lse.data_ptr(),
                                        scratch[R:2 * R].data_ptr(), scratch[2 * R:].data_ptr(), None), "s2vt_mean_ce_forward")
    return B, Lm1, R, logits, target, lse, torch.tensor([gout], dtype=torch.float32, device=DEV)


def _mean_ce_backward(lib, B, Lm1, V, logits, target, lse, gout):
    from s2vt_video_caption_amd import capi
    dlogits = torch.empty_like(logits)
    capi.check(lib.s2vt_mean_ce_backward(B, Lm1, V, logits.data_ptr(), target.data_ptr(), target.stride(0), lse.data_ptr(),
                                         gout.data_ptr(), dlogits.data_ptr(), None), "s2vt_mean_ce_backward")
    return dlogits


@pytest.mark.parametrize("gout", [1.0, 0.37])
@pytest.mark.parametrize("V", [70, 300])
def test_split_dual_ce_gradient_is_the_two_kernel_route(lib, V, gout):
    """The fused CE-gradient transform (3 planes) at R = 135 rows, no multiple of 64: planes and per-chunk column sums bit for
    bit those of s2vt_mean_ce_backward followed by the split / s2vt_colsum - the kernel's own claim."""
    from s2vt_video_caption_amd import ops
    B, Lm1, R, logits, target, lse, g = _ce_problem(lib, V, gout, seed=36)
    dlogits = _mean_ce_backward(lib, B, Lm1, V, logits, target, lse, g)
    assert bool(torch.isfinite(dlogits).all()) and float(dlogits.abs().max()) > 0
    res = ops.split_planes_dual(logits, 3, want_t=True, want_colpart=True, ce=dict(lse=lse, target=target, Lm1=Lm1, gout=g))
    assert _planes_equal(ops, res["r"], dlogits, 3)
    assert _planes_equal(ops, res["t"], dlogits, 3, transpose=True)
    total, partial = ops.colsum(dlogits)
    assert partial.shape == res["colpart"].shape == (3, V)
    assert _bitwise_equal(res["colpart"], partial)
    assert _bitwise_equal(ops.colsum_finish(res["colpart"]), total)


@pytest.mark.parametrize("gout", [1.0, 0.37])
@pytest.mark.parametrize("V", [70, 300])
def test_split_dual_ce_gradient_power_of_two_scale(lib, V, gout):
    """bf16 mode (1 plane, alpha_out): the planes carry the scale gout / rows as its power of two s2 only, alpha = scale / s2 in
    [1, 2) is handed out and multiplied into the column sums.  gout' = s2 * rows makes s2vt_mean_ce_backward's scale exactly s2."""
    from s2vt_video_caption_amd import ops
    B, Lm1, R, logits, target, lse, g = _ce_problem(lib, V, gout, seed=37)
    scale = np.float32(gout) / np.float32(R)
    s2 = (np.array([scale], dtype=np.float32).view(np.uint32) & np.uint32(0xFF800000)).view(np.float32)[0]
    alpha = np.float32(scale / s2)
    assert 1.0 <= alpha < 2.0 and math.frexp(float(s2))[0] == 0.5 and np.float32(alpha * s2) == scale
    g2 = torch.tensor([float(s2) * R], dtype=torch.float32, device=DEV)
    assert float(g2[0]) / R == float(s2)
    dl = _mean_ce_backward(lib, B, Lm1, V, logits, target, lse, g2)
    res = ops.split_planes_dual(logits, 1, want_t=True, want_colpart=True, ce=dict(lse=lse, target=target, Lm1=Lm1, gout=g, alpha=True))
    assert float(res["alpha"][0]) == float(alpha)
    assert _planes_equal(ops, res["r"], dl, 1)
    assert _planes_equal(ops, res["t"], dl, 1, transpose=True)
    _, partial = ops.colsum(dl)
    assert _bitwise_equal(res["colpart"], partial * torch.tensor(float(alpha), dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------------ colsum, gather_rows, transpose
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 4097, 4480])
def test_colsum_exact(lib, rows):
    """rows around one 64-row chunk; 4097 rows = 65 chunks, the first count at which colsum_final_kernel's four-accumulator loop
    runs (16 thread rows x 4); 4480 = 70 chunks.  cols around its 16-column workgroups; contiguous and strided rows."""
    from s2vt_video_caption_amd import ops
    for cols in (1, 15, 16, 17, 300):
        x = _ints(rows, cols, seed=40 + cols)
        total, chunks = x.long().sum(0).float(), _chunk_sums(x)
        pre = _ints(cols, seed=41)
        for ld in (cols, cols + 3):
            xd = torch.full((rows, ld), 77.0, device=DEV)
            xd[:, :cols] = x.to(DEV)
            out, partial = ops.colsum(xd[:, :cols])
            assert torch.equal(out.cpu(), total), (cols, ld)
            assert torch.equal(partial.cpu(), chunks), (cols, ld)
            out, _ = ops.colsum(xd[:, :cols], out=pre.to(DEV), accumulate=True)
            assert torch.equal(out.cpu(), pre + total), (cols, ld, "accumulate")


@pytest.mark.parametrize("cols", [1, 7, 40, 1028])
def test_gather_rows_exact(lib, cols):
    """cols = 40 / 1028 with ld = cols: 16-byte copies (1028: two thread blocks per row); ld = cols + 1 and the other widths: scalar"""
    from s2vt_video_caption_amd import ops
    V = 50
    idx = _idx(300, V, seed=42)
    for ld in (cols, cols + 1):
        src = _ints(V, ld, seed=43, lo=-1000, hi=1000)
        got = ops.gather_rows(src.to(DEV)[:, :cols], idx.int().to(DEV))
        assert torch.equal(got.cpu(), src[idx][:, :cols]), ld


@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 3), (130, 33), (4000, 1000), (3000, 1000)])
def test_transpose_exact(lib, rows, cols):
    """(4000, 1000) / (3000, 1000): W_hh of the LSTM and of the GRU at H = 1000"""
    from s2vt_video_caption_amd import ops
    x = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)          # every element distinct (< 2^24)
    assert torch.equal(ops.transpose(x.to(DEV)).cpu(), x.t().contiguous())

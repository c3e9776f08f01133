"""-m gpu: the forward launches between guard bands, on NaN-filled outputs and with strided operands.

Every case writes its result into a ``util.guarded`` buffer (front guard | rows x ld | back guard, every byte the NaN pattern): a store
outside the [rows, cols] result changes a guard or a pad column, an element the kernel skips stays NaN.  Where the op allocates its
own output, ``util.nan_fill_free`` runs immediately before the launch, so that the block the allocator hands out reads NaN instead of
the right numbers of an earlier call.  Strided cases embed the operands with ``util.poisoned_input`` (NaN pad columns, NaN rows behind
the last): bytes outside an operand that reach the result -- a K tail masked by multiplication, a row past M -- give NaN.

The numbers are compared with a float64 CPU restatement of the operation on the same operands at util.TOL[dtype] (the fused
sub-layers at the bound their tests in test_gpu_kernels.py use, 1.5 x TOL, window attention at clap_audio_models.TOL), per block of
64 rows so that a bad tail block is not hidden behind the maximum of the whole result.  GEMM operands come from util.exact_operand:
exact in bf16, f16 and fp32, so the three storage types and both fp32 matmul precisions ("high" splits a bf16-exact operand without
loss) share one reference.

Guards: util.GUARD_ROWS = 256 rows, the largest row tile of any kernel here (cgemm.hip CBM, hconv.hip BM; gemm.hip 128 / 64,
f32_ops.hip 64, rpgemm.hip / wsgemm.hip 32 rows per wave, mlp.hip 128, mlp3.hip / geglu3.hip 256, xattn.hip 128, attention.hip 64,
hsattn.hip 64, norm.hip 4 rows per workgroup); the element-wise cases say their own."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from util import TOL, block_rel_err, exact_operand as E, guarded, nan_buffer, nan_fill_free, poisoned_input, q

pytestmark = pytest.mark.gpu
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES16 = [BF, HF]
DTYPES = [BF, HF, F32]
MODES = [(BF, None), (HF, None), (F32, "highest"), (F32, "high")]  # (storage type, fp32 matmul precision)
MODE_IDS = ["bf16", "f16", "f32-highest", "f32-high"]


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """scratch and side outputs the wrappers allocate themselves (row statistics, workspaces) come from NaN-filled blocks too"""
    nan_fill_free(dev)
    yield


@contextlib.contextmanager
def precision(prec):
    from ap_adapter_amd import ops
    old = ops.get_float32_matmul_precision()
    if prec is not None:
        ops.set_float32_matmul_precision(prec)
    try:
        yield
    finally:
        ops.set_float32_matmul_precision(old)


@contextlib.contextmanager
def gemm_ring(mode):
    from ap_adapter_amd import ops
    old = ops.set_gemm_ring(mode)
    try:
        yield
    finally:
        ops.set_gemm_ring(old)


def close(out, ref, tol, what="", bm=64):
    """finite everywhere, and every block of ``bm`` rows (the ragged last one on its own) within tol of that block's max|ref|"""
    ref = ref.detach().double().cpu()
    o = out.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite values in the result"
    M = ref.shape[0]
    o, ref = o.reshape(M, -1), ref.reshape(M, -1)
    full = M // bm
    worst = []
    if full:
        worst.append(block_rel_err(o[:full * bm], ref[:full * bm], full))
    if M % bm:
        worst.append((block_rel_err(o[full * bm:], ref[full * bm:], 1)[0], full))
    e, i = max(worst)
    print(f"{what}: worst row block {i} rel_err {e:.3e} (bound {tol:g})")
    assert e < tol, f"{what}: rows {i * bm}..{min(M, (i + 1) * bm) - 1}: rel_err {e:.3e} >= {tol:g}"


def full_width(view):
    """the [rows, ld] tensor over a strided [rows, cols] view (for the wrappers that take a row stride from ``shape[-1]``)"""
    return view.as_strided((view.shape[0], view.stride(0)), (view.stride(0), 1))


def gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def ln64(x, g, b, eps):
    x = x.double()
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


# ---------------------------------------------------------------------------------------------------------------------------------
# apad_gemm, plain A
# ---------------------------------------------------------------------------------------------------------------------------------
EPILOGUES = [None, "bias_res", "silu", "gelu", "geglu"]


@functools.lru_cache(maxsize=None)
def _gemm_operands(M, N, K):
    x, w, b, r = E(M, K, seed=1), E(2 * N, K, seed=2, std=0.05), E(2 * N, seed=3), E(M, N, seed=4)
    y = x.double() @ w.double().t()
    yb = y + b.double()
    ref = {None: y[:, :N], "bias_res": yb[:, :N] + r.double(), "silu": F.silu(yb[:, :N]), "gelu": gelu64(yb[:, :N]),
           "geglu": yb[:, :N] * gelu64(yb[:, N:])}
    return x, w, b, r, ref


def _gemm_case(dev, dtype, prec, M, N, K, ring=0):
    """dense, then lda = K + 8, ldw = K + 8, ldo = N + 8, ldr = N + 16 on poisoned operands; every epilogue the shape admits; the
    row statistics (16-bit, N % 64 == 0, no GEGLU) in a guarded buffer of their own"""
    from ap_adapter_amd import ops, _lib as L
    x, w, b, r, ref = _gemm_operands(M, N, K)
    D = lambda t: t.to(dev, dtype)
    geglu_n = 32 if dtype == F32 else 64  # the ABI's GEGLU envelope: N % (8 vectors) == 0
    x3_before, launches = int(L.lib().apad_f32x3_launch_count()), 0
    with precision(prec), gemm_ring(ring):
        for strided in (False, True):
            if strided:
                xa, w1, w2, ra = (poisoned_input(D(x), K + 8), poisoned_input(D(w[:N]), K + 8), poisoned_input(D(w), K + 8),
                                  poisoned_input(D(r), N + 16))
            else:
                xa, w1, w2, ra = D(x), D(w[:N]), D(w), D(r)
            ldo = N + 8 if strided else N
            for epi in EPILOGUES:
                if epi == "geglu" and N % geglu_n:
                    continue
                what = f"gemm {M}x{N}x{K} {dtype} {prec} ring={ring} strided={strided} epilogue={epi}"
                out, check = guarded(M, N, dtype, dev, ld=ldo)
                kw = {}
                if epi == "bias_res":
                    kw = dict(bias=D(b[:N]), residual=ra, ldr=ra.stride(0))
                elif epi == "geglu":
                    kw = dict(bias=D(b), act="geglu")
                elif epi is not None:
                    kw = dict(bias=D(b[:N]), act=epi)
                wa = w2 if epi == "geglu" else w1
                ops.gemm(xa, wa, M=M, N=N, K=K, lda=xa.stride(0), out=out, ldo=ldo, ldw=wa.stride(0), **kw)
                launches += 1
                check(what)
                close(out, ref[epi], TOL[dtype], what)
                if dtype in DTYPES16 and N % 64 == 0 and epi != "geglu":
                    # the same launch with the row statistics as a side output (a launch of its own: the big-tile form emits none):
                    # (sum, sum of squares) per 64 columns of the STORED row (include/apadapter_hip.h)
                    out, check = guarded(M, N, dtype, dev, ld=ldo)
                    rs, rs_check = guarded(M, 2 * (N // 64), F32, dev)
                    ops.gemm(xa, wa, M=M, N=N, K=K, lda=xa.stride(0), out=out, ldo=ldo, ldw=wa.stride(0), rowstat_out=rs, **kw)
                    check(what + " + rowstat_out")
                    rs_check(what + " rowstat_out")
                    close(out, ref[epi], TOL[dtype], what + " + rowstat_out")
                    o = out.double().cpu().view(M, N // 64, 64)
                    close(rs, torch.stack([o.sum(-1), (o * o).sum(-1)], -1).view(M, -1), TOL[F32], what + " rowstat_out")
    # the route: "high" ran every launch on the bf16x3 kernel, the other modes none
    assert int(L.lib().apad_f32x3_launch_count()) - x3_before == (launches if prec == "high" else 0)


# (77, 8, 72): N below a vector tile, K no multiple of the k-tile; (130, 72, 136): three 64-row tiles, ragged N and K;
# (513, 640, 64): one k-tile, ten column tiles, a one-row last tile; (32777, 128, 64): the big-tile form (cgemm.hip: 16-bit, from
# 16000 rows, N % 128 == 0, epilogue NONE) with a 9-row last tile
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("M,N,K", [(77, 8, 72), (130, 72, 136), (513, 640, 64), (32777, 128, 64)])
def test_gemm_plain(dev, mode, M, N, K):
    _gemm_case(dev, mode[0], mode[1], M, N, K)


# the LDS-DMA ring form (gemm.hip launch_ring: K >= 128, K % 64 == 0, N % 64 == 0, below 16000 rows; epilogue NONE / GEGLU):
# (130, 128, 192) three k-tiles, (513, 640, 384) the two-K-group variant
@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("M,N,K", [(130, 128, 192), (513, 640, 384)])
def test_gemm_ring_form(dev, dtype, M, N, K):
    _gemm_case(dev, dtype, None, M, N, K, ring=2)


# two A sources, the smaller batch read modulo: M = 130, K = 64 + 72 (tiled kernel), K = 64 + 64 on the ring form
@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("Ca,Cb,N,ring", [(64, 72, 72, 0), (64, 64, 64, 2)])
def test_linear2_modulo_batch(dev, dtype, Ca, Cb, N, ring):
    from ap_adapter_amd import ops
    Ba, Bb, T = 2, 1, 65
    xa, xb, w, b = E(Ba, T, Ca, seed=5), E(Bb, T, Cb, seed=6), E(N, Ca + Cb, seed=7, std=0.05), E(N, seed=8)
    cat = torch.cat([xa, xb.repeat(Ba, 1, 1)], -1).double()
    ref = (cat @ w.double().t() + b.double()).view(Ba * T, N)
    D = lambda t: t.to(dev, dtype)
    out, check = guarded(Ba * T, N, dtype, dev)
    with gemm_ring(ring):
        ops.linear2(D(xa), D(xb), D(w), D(b), out=out.view(Ba, T, N))
    check("linear2")
    close(out, ref, TOL[dtype], f"linear2 K={Ca}+{Cb} ring={ring}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-head column-slice launches of text_encoders.py / vae.py
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("d", [32, 48, 64, 80])
def test_gemm_per_head_slices(dev, mode, d):
    """q_h . k_h^T with lda = ldw = C, P . V_h with ldw = Lpad into the head's columns of [L, C] (ldo = C: the other heads' columns,
    pre-filled with a pattern, stay bit-unchanged), and the q | k split of one [L, 2C] buffer (lda = ldw = 2C).  40 tokens, 3 heads,
    the middle head: its neighbours' columns lie on both sides of every row."""
    from ap_adapter_amd import ops
    dtype, prec = mode
    heads, Lk, h = 3, 40, 1
    C, Lpad = heads * d, 64
    cols = slice(h * d, (h + 1) * d)
    qq, kk, pp, vv = E(Lk, C, seed=11), E(Lk, C, seed=12), E(Lk, Lk, seed=13, std=0.2), E(Lk, C, seed=14)
    D = lambda t: t.to(dev, dtype)
    with precision(prec):
        # scores: K = d (48 and 80 are no multiples of the k-tile: the tail lies in the next head's columns)
        out, check = guarded(Lk, Lk, dtype, dev)
        qd, kd = D(qq), D(kk)
        ops.gemm(qd[:, cols], kd[:, cols], M=Lk, N=Lk, K=d, lda=C, ldw=C, out=out, ldo=Lk)
        check("q_h . k_h^T")
        close(out, qq[:, cols].double() @ kk[:, cols].double().t(), TOL[dtype], f"q_h . k_h^T d={d}")
        # P . V_h: the A rows and the V^T rows padded with NaN (K = 40 ends inside a k-tile on both operands)
        pa = poisoned_input(D(pp), Lk + 8)
        vt = poisoned_input(D(vv[:, cols].t().contiguous()), Lpad)
        o2, check = guarded(Lk, C, dtype, dev)
        pattern = D(((torch.arange(Lk * C) % 251).float() / 256.0 + 0.5).view(Lk, C))
        o2.copy_(pattern)
        ops.gemm(pa, vt, M=Lk, N=d, K=Lk, lda=pa.stride(0), ldw=Lpad, out=o2[:, cols], ldo=C)
        check("P . V_h")
        close(o2[:, cols], pp.double() @ vv[:, cols].double(), TOL[dtype], f"P . V_h d={d}")
        keep = torch.ones(C, dtype=torch.bool)
        keep[cols] = False
        assert torch.equal(o2[:, keep.to(dev)], pattern[:, keep.to(dev)]), "P . V_h changed another head's columns"
        # q | k halves of one buffer
        qk = D(torch.cat([qq, kk], -1))
        out, check = guarded(Lk, Lk, dtype, dev)
        ops.gemm(qk[:, :C], qk[:, C:], M=Lk, N=Lk, K=C, lda=2 * C, ldw=2 * C, out=out, ldo=Lk)
        check("q . k^T over the q | k split")
        close(out, qq.double() @ kk.double().t(), TOL[dtype], f"q . k^T lda=2C C={C}")


# ---------------------------------------------------------------------------------------------------------------------------------
# V^T and fused q | k | v outputs: only l < L of each [Lpad] row is written (ops.linear_vt: "zero padded by the caller; only l < Lk is
# written"), so the pad columns L..Lpad keep the caller's bytes -- here the guard pattern -- and nothing beyond Lpad is touched
# ---------------------------------------------------------------------------------------------------------------------------------
def _vt_guarded(B, heads, d, Lk, Lpad, dtype, dev):
    view, check = guarded(B * heads * d, Lk, dtype, dev, ld=Lpad)
    return view, full_width(view).view(B, heads, d, Lpad), check


def _vt_ref(y, B, Lk, heads, d):
    return y.view(B, Lk, heads, d).permute(0, 2, 3, 1).reshape(B * heads * d, Lk)


VT_L = [8, 33, 100, 513]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("Lk", VT_L)
def test_linear_vt(dev, mode, Lk):
    from ap_adapter_amd import ops
    dtype, prec = mode
    B, heads, d, K = 2, 2, 32, 64
    C = heads * d
    x, w, b = E(B * Lk, K, seed=21), E(C, K, seed=22, std=0.1), E(C, seed=23)
    D = lambda t: t.to(dev, dtype)
    Lpad = ops.round_up(Lk, 32)
    view, vt, check = _vt_guarded(B, heads, d, Lk, Lpad, dtype, dev)
    with precision(prec):
        ops.linear_vt(poisoned_input(D(x), K + 8), D(w), B, Lk, heads, vt, bias=D(b))
    check(f"linear_vt L={Lk}")
    close(view, _vt_ref(x.double() @ w.double().t() + b.double(), B, Lk, heads, d), TOL[dtype], f"linear_vt L={Lk}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("Lk", VT_L)
def test_linear_qkv(dev, mode, Lk):
    """the tiled kernel's q | k | v^T output mode (C = 128: a column tile lies in one third), with the row-major v copy"""
    from ap_adapter_amd import ops
    dtype, prec = mode
    B, heads, d, K = 2, 4, 32, 64
    C, M = heads * d, B * Lk
    x, w = E(M, K, seed=24), E(3 * C, K, seed=25, std=0.1)
    y = x.double() @ w.double().t()
    D = lambda t: t.to(dev, dtype)
    Lpad = ops.round_up(Lk, 32)
    view, vt, check = _vt_guarded(B, heads, d, Lk, Lpad, dtype, dev)
    (qo, qc), (ko, kc), (vo, vc) = (guarded(M, C, dtype, dev) for _ in range(3))
    with_v = dtype in DTYPES16  # (the row-major v copy is the 16-bit training step's; the fp32 path has no such output)
    with precision(prec):
        ops.linear_qkv(poisoned_input(D(x), K + 8), D(w), B, Lk, heads, qo, ko, vt, v=vo if with_v else None)
    for c, name in ((qc, "q"), (kc, "k"), (check, "v^T")) + (((vc, "v"),) if with_v else ()):
        c(f"linear_qkv L={Lk} {name}")
    close(qo, y[:, :C], TOL[dtype], "linear_qkv q")
    close(ko, y[:, C:2 * C], TOL[dtype], "linear_qkv k")
    close(view, _vt_ref(y[:, 2 * C:], B, Lk, heads, d), TOL[dtype], "linear_qkv v^T")
    if with_v:
        assert torch.equal(_vt_ref(vo, B, Lk, heads, d), view.contiguous()), "row-major v and v^T differ"


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("Lk", VT_L)
def test_rowpanel_vt_segment(dev, dtype, Lk):
    """LayerNorm + q | k | v^T on the row-panel kernel (rp_shared.h scratch_flush_vt: 16-byte, 8-byte and element stores by alignment)"""
    from ap_adapter_amd import ops
    B, heads, K = 2, 8, 256
    d, M = K // heads, B * Lk
    x, w = E(M, K, seed=26, shift=0.2), E(3 * K, K, seed=27, std=0.06)
    g, be = E(K, seed=28, std=0.1, shift=1.0), E(K, seed=29, std=0.1)
    y = q(ln64(x, g, be, 1e-5).float(), dtype).double() @ w.double().t()
    D = lambda t: t.to(dev, dtype)
    Lpad = ops.round_up(Lk, 32)
    view, vt, check = _vt_guarded(B, heads, d, Lk, Lpad, dtype, dev)
    (qo, qc), (ko, kc) = (guarded(M, K, dtype, dev) for _ in range(2))
    ops.rowpanel(poisoned_input(D(x), K + 8), D(w), [(qo, None, K, "row"), (ko, None, K, "row"), (vt, None, K, "vt")],
                 ln=(D(g), D(be), 1e-5), vt_geom=(heads, d, Lk, Lpad))
    for c, name in ((qc, "q"), (kc, "k"), (check, "v^T")):
        c(f"rowpanel L={Lk} {name}")
    close(qo, y[:, :K], TOL[dtype], "rowpanel q")
    close(ko, y[:, K:2 * K], TOL[dtype], "rowpanel k")
    close(view, _vt_ref(y[:, 2 * K:], B, Lk, heads, d), TOL[dtype], "rowpanel v^T")


# ---------------------------------------------------------------------------------------------------------------------------------
# row-panel: the weight-stationary kernel (wsgemm.hip: up to 512 output columns, no GEGLU) and the streamed-tile kernel (rpgemm.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("M", [17, 37, 257])
def test_rowpanel(dev, dtype, M, K):
    """one / two / three segments into outputs wider than n_cols (ldo = n_cols + 64), x and w rows padded with NaN (lda = ldw = K + 8),
    with and without LayerNorm, residual (ldr = N + 16) and GEGLU"""
    from ap_adapter_amd import ops
    N = K
    x, w, b, r = E(M, K, seed=31, shift=0.2), E(3 * N, K, seed=32, std=0.05), E(3 * N, seed=33, std=0.3), E(M, N, seed=34)
    g, be = E(K, seed=35, std=0.1, shift=1.0), E(K, seed=36, std=0.1)
    D = lambda t: t.to(dev, dtype)
    xa, wa = poisoned_input(D(x), K + 8), poisoned_input(D(w), K + 8)
    ra = full_width(poisoned_input(D(r), N + 16))
    lnp = (D(g), D(be), 1e-5)
    x64 = {False: x.double(), True: q(ln64(x, g, be, 1e-5).float(), dtype).double()}
    y = {k: v @ w.double().t() + b.double() for k, v in x64.items()}

    def seg(n):
        view, check = guarded(M, n, dtype, dev, ld=n + 64)
        return view, full_width(view), check

    for ln in (False, True):
        what = f"rowpanel M={M} K={K} ln={ln}"
        # one segment + bias (+ residual when ln): the weight-stationary kernel
        view, wide, check = seg(N)
        ops.rowpanel(xa, wa[:N], [(wide, D(b[:N]), N, "row")], ln=lnp if ln else None, residual=ra if ln else None)
        check(what + " one segment")
        close(view, y[ln][:, :N] + (r.double() if ln else 0), TOL[dtype], what + " one segment")
        # GEGLU: the streamed-tile kernel
        view, wide, check = seg(N)
        ops.rowpanel(xa, wa[:2 * N], [(wide, D(b[:2 * N]), N, "row")], ln=lnp if ln else None, act="geglu")
        check(what + " geglu")
        close(view, y[ln][:, :N] * gelu64(y[ln][:, N:2 * N]), TOL[dtype], what + " geglu")
        # two (K = 256: 512 columns, weight-stationary; K = 384: streamed) and three segments
        for nseg in (2, 3):
            segs = [seg(N) for _ in range(nseg)]
            bias = [D(b[i * N:(i + 1) * N]) for i in range(nseg)]
            ops.rowpanel(xa, wa[:nseg * N], [(s[1], bias[i], N, "row") for i, s in enumerate(segs)], ln=lnp if ln else None)
            for i, (view, _, check) in enumerate(segs):
                check(f"{what} segment {i} of {nseg}")
                close(view, y[ln][:, i * N:(i + 1) * N], TOL[dtype], f"{what} segment {i} of {nseg}")


# ---------------------------------------------------------------------------------------------------------------------------------
# conv3x3 / conv1d: one case per kernel form, that form's smallest shape in test_gpu_kernels.py / test_gpu_vae.py / test_gpu_vocoder.py
# ---------------------------------------------------------------------------------------------------------------------------------
def _conv3x3_case(dev, dtype, prec, B, H, W, Cin, Cout, stride=1, up=None, asym=False, residual=False, halo=None):
    from ap_adapter_amd import ops, _lib as L
    x, w, b = E(B, Cin, H, W, seed=41), E(Cout, Cin, 3, 3, seed=42, std=0.05), E(Cout, seed=43)
    t = x.double()
    if up is not None:
        t = F.interpolate(t, size=up, mode="nearest")
    t = F.pad(t, (0, 1, 0, 1)) if asym else F.pad(t, (1, 1, 1, 1))
    ref = F.conv2d(t, w.double(), b.double(), stride=stride)
    Ho, Wo = ref.shape[2:]
    ref = ref.permute(0, 2, 3, 1).reshape(B * Ho * Wo, Cout)
    D = lambda a: a.to(dev, dtype)
    kw = {}
    if residual:
        r = E(B * Ho * Wo, Cout, seed=44)
        ref = q(ref.float(), dtype).double() + r.double()  # (the kernels round the convolution to the storage type before the add)
        kw["residual"] = D(r).view(B, Ho * Wo, Cout)
    out, check = guarded(B * Ho * Wo, Cout, dtype, dev)
    xn = D(x.permute(0, 2, 3, 1).reshape(B, H * W, Cin).contiguous())
    wp = D(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous())
    n0 = L.lib().apad_hconv_launch_count()
    with precision(prec):
        _, Ho2, Wo2 = ops.conv3x3(xn, wp, D(b), B, H, W, stride=stride, up=up, asym_pad=asym, out=out.view(B, Ho * Wo, Cout), **kw)
    if halo is not None:
        assert (L.lib().apad_hconv_launch_count() == n0 + 1) == halo, "halo kernel route"
    assert (Ho2, Wo2) == (Ho, Wo)
    what = f"conv3x3 {B}x{H}x{W} {Cin}->{Cout} stride={stride} up={up} asym={asym} {dtype} {prec}"
    check(what)
    close(out, ref, TOL[dtype], what)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up,asym", [
    (2, 10, 16, 8, 128, 1, None, False),      # implicit GEMM on the tiled kernel (Cin = 8: the general gather), 320 pixels
    (2, 25, 16, 128, 128, 2, None, False),    # stride 2 (Cin % 64 == 0: the fast gather), 13 x 8 output pixels per sample
    (2, 13, 8, 64, 96, 1, (26, 16), False),   # nearest-up-sampled source
    (1, 21, 9, 32, 64, 2, None, True),        # asymmetric padding, odd image
])
def test_conv3x3_tiled_forms(dev, mode, B, H, W, Cin, Cout, stride, up, asym):
    _conv3x3_case(dev, mode[0], mode[1], B, H, W, Cin, Cout, stride, up, asym, halo=False)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("B,H,W,Cin,Cout,up,residual,halo", [
    (1, 5, 4, 64, 128, None, True, True),     # halo-resident kernel, wide form: one sample smaller than a 256-row tile
    (3, 5, 4, 64, 128, None, True, True),     # ... sample boundaries inside the tile
    (5, 63, 4, 64, 16, None, False, True),    # halo narrow form (Cout <= 16), ragged last tile
    (1, 9, 7, 256, 64, None, True, False),    # small-tile LDS-DMA ring (cgemm.hip, K = 2304, 63 of 64 rows)
    (3, 63, 4, 384, 384, None, True, True),   # 756 pixels = 2.95 tiles, three column tiles
])
def test_conv3x3_dma_forms(dev, dtype, B, H, W, Cin, Cout, up, residual, halo):
    _conv3x3_case(dev, dtype, None, B, H, W, Cin, Cout, up=up, residual=residual, halo=halo)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B,T,Cin,Cout,k,dil,s,act", [
    (2, 50, 64, 128, 7, 1, 0, None),    # Conv1d, "same" padding, + pre-activation + residual
    (1, 77, 32, 32, 11, 5, 0, None),    # dilation 5: 25 zero taps on either side
    (1, 40, 32, 8, 7, 1, 0, "tanh"),    # conv_post: one channel padded to Cout = 8, tanh
    (2, 37, 64, 32, 16, 5, 5, None),    # ConvTranspose1d, k - s odd: output 5 T + 1
    (2, 61, 32, 16, 4, 2, 2, None),     # ConvTranspose1d, k - s even
])
def test_conv1d(dev, mode, B, T, Cin, Cout, k, dil, s, act):
    from ap_adapter_amd import ops
    dtype, prec = mode
    x, b = E(B, Cin, T, seed=45), E(Cout, seed=47, std=0.1)
    D = lambda a: a.to(dev, dtype)
    xl = D(x.transpose(1, 2).contiguous())
    if s:
        w = E(Cin, Cout, k, seed=46, std=0.05)
        ref = F.conv_transpose1d(F.leaky_relu(x.double(), 0.1), w.double(), b.double(), stride=s, padding=(k - s) // 2)
        wp, kw = D(w.permute(1, 2, 0).reshape(Cout, -1).contiguous()), dict(transposed_stride=s, pre_slope=0.1)
    else:
        w = E(Cout, Cin, k, seed=46, std=0.05)
        pre = act is None
        ref = F.conv1d(F.leaky_relu(x.double(), 0.1) if pre else x.double(), w.double(), b.double(), dilation=dil, padding=(k * dil - dil) // 2)
        wp, kw = D(w.permute(0, 2, 1).reshape(Cout, -1).contiguous()), dict(dilation=dil, pre_slope=0.1 if pre else None, act=act)
    Tout = ref.shape[2]
    ref = ref.transpose(1, 2).reshape(B * Tout, Cout)
    if act == "tanh":
        ref = torch.tanh(ref)
    elif not s:
        r = E(B * Tout, Cout, seed=48)
        ref = q(ref.float(), dtype).double() + r.double()
        kw["residual"] = D(r).view(B, Tout, Cout)
    out, check = guarded(B * Tout, Cout, dtype, dev)
    with precision(prec):
        ops.conv1d(xl, wp, D(b), k, out=out.view(B, Tout, Cout), **kw)
    what = f"conv1d T={T} {Cin}->{Cout} k={k} dil={dil} s={s} act={act} {dtype} {prec}"
    check(what)
    close(out, ref, TOL[dtype], what)


# ---------------------------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [256, 768, 1280])  # norm.hip ln_launch: 1, 2, 4 vectors per lane
@pytest.mark.parametrize("M", [1, 7, 130])       # 4 rows per workgroup: a one-row grid, a ragged one, 32.5 workgroups
def test_layer_norm_strides(dev, dtype, M, C):
    """apad_layernorm called directly (ops.layer_norm exposes no row stride): dense, then ldx = C + 8, ldo = C + 16"""
    from ap_adapter_amd import ops, _lib as L
    x, g, b = E(M, C, seed=51, std=2.0, shift=0.5), E(C, seed=52, std=0.1, shift=1.0), E(C, seed=53, std=0.1)
    D = lambda t: t.to(dev, dtype)
    gd, bd = D(g), D(b)
    for ldx, ldo in ((C, C), (C + 8, C + 16)):
        xa = poisoned_input(D(x), ldx)
        out, check = guarded(M, C, dtype, dev, ld=ldo)
        L.check(L.lib().apad_layernorm(xa.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, C, ldx, ldo, 1e-5, ops._DT[dtype],
                                       ops._stream()), "apad_layernorm")
        what = f"layer_norm M={M} C={C} ldx={ldx} ldo={ldo} {dtype}"
        check(what)
        close(out, ln64(x, g, b, 1e-5), TOL[dtype], what)


# norm.hip gn_launch with 32 groups: C = 256 / 128 the 512-thread full-line forms (cg = 8 / 4), C = 384 the default one-pass forms
# (256 threads x 24 vectors up to 1008 pixels, 1024 x 12 above), HW = 1025 the two-pass form: C = 256 its division-free loop
# (256 % vpr == 0), C = 384 the generic one (vpr = 48)
GN_CASES = [(100, 256, True), (100, 128, False), (63, 384, True), (1013, 384, False), (1025, 256, True), (1025, 384, False)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW,C,silu", GN_CASES)
def test_group_norm_forms(dev, dtype, HW, C, silu):
    from ap_adapter_amd import ops
    B = 3
    x, g, b = E(B, HW, C, seed=54, std=1.5, shift=0.3), E(C, seed=55, std=0.1, shift=1.0), E(C, seed=56, std=0.1)
    ref = F.group_norm(x.double().transpose(1, 2), 32, g.double(), b.double(), 1e-5).transpose(1, 2)
    ref = F.silu(ref) if silu else ref
    D = lambda t: t.to(dev, dtype)
    out, check = guarded(B * HW, C, dtype, dev)
    ops.group_norm(D(x), D(g), D(b), 32, 1e-5, silu=silu, out=out.view(B, HW, C))
    what = f"group_norm HW={HW} C={C} silu={silu} {dtype}"
    check(what)
    close(out, ref.reshape(B * HW, C), TOL[dtype], what)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("HW,Ca,Cb,silu", [(63, 256, 128, True), (1025, 256, 128, False)])  # one-pass and two-pass, 12-channel groups
def test_group_norm2(dev, dtype, HW, Ca, Cb, silu):
    """allocates its own output: NaN-filled free memory immediately before the launch"""
    from ap_adapter_amd import ops
    B, Bb = 3, 1
    xa, xb = E(B, HW, Ca, seed=57, shift=0.3), E(Bb, HW, Cb, seed=58, std=2.0)
    C = Ca + Cb
    g, b = E(C, seed=59, std=0.2, shift=1.0), E(C, seed=60, std=0.2)
    cat = torch.cat([xa, xb.repeat(B, 1, 1)], -1).double()
    ref = F.group_norm(cat.transpose(1, 2), 32, g.double(), b.double(), 1e-5).transpose(1, 2)
    ref = F.silu(ref) if silu else ref
    D = lambda t: t.to(dev, dtype)
    ops_in = D(xa), D(xb), D(g), D(b)
    nan_fill_free(dev)
    out = ops.group_norm2(*ops_in, 32, 1e-5, silu=silu)
    close(out.view(B * HW, C), ref.reshape(B * HW, C), TOL[dtype], f"group_norm2 HW={HW} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 63, 257])
def test_softmax_rows_strides(dev, dtype, N):
    """ldx = N + 5, ldb = N + 3, ldo = N + 7 (one wave per row, four rows per workgroup: M = 37 leaves a ragged last workgroup)"""
    from ap_adapter_amd import ops
    M = 37
    x, bias = E(M, N, seed=61, std=4.0), E(M, N, seed=62)
    ref = torch.softmax(x.double() * 0.37 + bias.double(), -1)
    xa, ba = poisoned_input(x.to(dev, dtype), N + 5), poisoned_input(bias.to(dev), N + 3)
    out, check = guarded(M, N, dtype, dev, ld=N + 7)
    ops.softmax_rows(xa, 0.37, out=out, bias=ba)
    check(f"softmax_rows N={N}")
    close(out, ref, TOL[dtype], f"softmax_rows N={N} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rms_norm_and_l2_normalize_on_a_strided_x(dev, dtype):
    from ap_adapter_amd import ops
    M, C = 37, 96
    x, g = E(M, C, seed=63, std=3.0), E(C, seed=64, std=0.1, shift=1.0)
    xa, gd = poisoned_input(x.to(dev, dtype), C + 8), g.to(dev, dtype)
    x64 = x.double()
    nan_fill_free(dev)
    out = ops.rms_norm(xa, gd, 1e-6)
    close(out, x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + 1e-6) * g.double(), TOL[dtype], f"rms_norm {dtype}")
    nan_fill_free(dev)
    out = ops.l2_normalize(xa)
    close(out, x64 / x64.norm(dim=-1, keepdim=True).clamp_min(1e-12), TOL[dtype], f"l2_normalize {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------------
# apad_attention: every stride of the descriptor differs from the dense one
# ---------------------------------------------------------------------------------------------------------------------------------
def _heads(x, h):
    b, n, c = x.shape
    return x.view(b, n, h, c // h).transpose(1, 2)


def _attn64(qq, kk, vv, heads, bias=None):
    qh, kh, vh = (_heads(t.double(), heads) for t in (qq, kk, vv))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    B, N = qq.shape[:2]
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, N, -1), s


def _strided_rows(t, dev, dtype, row_pad=3, col_pad=16, col0=8):
    """t [B, N, C] as a batch slice [1:] and column slice [col0 : col0 + C] of a NaN [B + 1, N + row_pad, C + col_pad] buffer"""
    B, N, C = t.shape
    wide = nan_buffer((B + 1) * (N + row_pad) * (C + col_pad), dtype, dev).view(B + 1, N + row_pad, C + col_pad)
    v = wide[1:, :N, col0:col0 + C]
    v.copy_(t.to(dev, dtype))
    return v


def _strided_vt(v, heads, Lpad, dev, dtype):
    """v [B, L, C] -> zero-padded V^T [B, heads, d, Lpad] whose batch stride is 16 elements (NaN) longer than dense"""
    B, Lk, C = v.shape
    n = heads * (C // heads) * Lpad
    flat = poisoned_input(torch.zeros(B, n, dtype=dtype, device=dev), n + 16, tail_rows=0)
    vt = flat.view(B, heads, C // heads, Lpad)
    vt[..., :Lk] = _heads(v, heads).transpose(-1, -2).to(dev, dtype)
    return vt


def _guarded_bnc(B, N, C, dtype, dev, row_pad=3, col_pad=16):
    """a [B, N, C] output whose batch and row strides differ from dense, inside ONE guarded buffer: rows b * (N + row_pad) + n of a
    [B * (N + row_pad) - row_pad, C] view with ld = C + col_pad.  The row_pad rows between two samples are pre-set to 1 and must
    still be 1 afterwards (check() itself wants them finite)."""
    rows = B * (N + row_pad) - row_pad
    view, check = guarded(rows, C, dtype, dev, ld=C + col_pad)
    gap = torch.ones(rows, dtype=torch.bool)
    for b in range(B):
        gap[b * (N + row_pad):b * (N + row_pad) + N] = False
    view[gap.to(dev)] = 1.0
    out = view.as_strided((B, N, C), ((N + row_pad) * (C + col_pad), C + col_pad, 1))

    def check_all(what):
        check(what)
        if bool(gap.any()):
            assert bool((view[gap.to(dev)] == 1.0).all()), f"{what}: rows between two samples of the output were written"

    return out, check_all


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("d", [32, 48, 64, 80])
@pytest.mark.parametrize("N", [1, 33, 777])
def test_attention_strides(dev, mode, N, d):
    """single segment (N = 777 with 300 keys at d = 32: the two-query-tile kernel), masked, decoupled text + audio; q and out column and
    batch slices of wider buffers, k rows and the V^T batches padded"""
    from ap_adapter_amd import ops
    dtype, prec = mode
    B, heads = 2, 2
    C = heads * d
    qq = E(B, N, C, seed=71)
    qd = _strided_rows(qq, dev, dtype)

    def kv(Lk, seed):
        k, v = E(B, Lk, C, seed=seed), E(B, Lk, C, seed=seed + 1)
        return k, v, _strided_rows(k, dev, dtype, row_pad=2, col_pad=8, col0=0), _strided_vt(v, heads, ops.round_up(Lk, 32), dev, dtype)

    with precision(prec):
        # single segment
        Lk = 300 if N == 777 else 33
        k, v, kd, vt = kv(Lk, 72)
        out, check = _guarded_bnc(B, N, C, dtype, dev)
        ops.attention(qd, kd, vt, Lk, heads, out=out)
        what = f"attention N={N} L={Lk} d={d} {dtype} {prec}"
        check(what)
        close(out.reshape(B * N, C), _attn64(qq, k, v, heads)[0].reshape(B * N, C), TOL[dtype], what)
        # masked
        Lk = 40
        k, v, kd, vt = kv(Lk, 74)
        bias = torch.zeros(B, Lk)
        bias[1::2, -4:] = -10000.0
        bias[0, 1] = -3.0
        out, check = _guarded_bnc(B, N, C, dtype, dev)
        ops.attention(qd, kd, vt, Lk, heads, key_bias=bias.to(dev), out=out)
        what = f"attention masked N={N} d={d} {dtype} {prec}"
        check(what)
        close(out.reshape(B * N, C), _attn64(qq, k, v, heads, bias)[0].reshape(B * N, C), TOL[dtype], what)
        # decoupled: 8 text + 33 audio keys
        k1, v1, k1d, vt1 = kv(8, 76)
        k2, v2, k2d, vt2 = kv(33, 78)
        out, check = _guarded_bnc(B, N, C, dtype, dev)
        ops.attention(qd, k1d, vt1, 8, heads, k2=k2d, vt2=vt2, L2=33, scale2=0.55, out=out)
        what = f"attention decoupled N={N} d={d} {dtype} {prec}"
        check(what)
        ref = _attn64(qq, k1, v1, heads)[0] + 0.55 * _attn64(qq, k2, v2, heads)[0]
        close(out.reshape(B * N, C), ref.reshape(B * N, C), TOL[dtype], what)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("N,Lk", [(33, 40), (777, 300)])
def test_attention_lse_side_output(dev, dtype, N, Lk):
    """the descriptor of ops.attention_lse filled here, so that the log-sum-exp [B, heads, round_up(N, 32)] lies in a guarded buffer
    too (the wrapper allocates it itself): every entry written, the pad entries exactly 0 ("the kernels write the pad entries: 0"),
    the rest at the bound of the existing lse test (1e-3); then the wrapper itself on NaN-filled free memory, bit-equal"""
    import ctypes
    from ap_adapter_amd import ops, _lib as L
    B, heads, d = 2, 2, 32
    C = heads * d
    Npad = ops.round_up(N, 32)
    qq, k, v = E(B, N, C, seed=81), E(B, Lk, C, seed=82), E(B, Lk, C, seed=83)
    D = lambda t: t.to(dev, dtype)
    qd, kd, vt = D(qq), D(k), _strided_vt(v, heads, ops.round_up(Lk, 32), dev, dtype).contiguous()
    ref, s = _attn64(qq, k, v, heads)
    out, check = guarded(B * N, C, dtype, dev)
    lse, lse_check = guarded(B * heads, Npad, F32, dev)
    desc = L.AttnDesc()
    desc.q, desc.k, desc.vt, desc.out, desc.lse = qd.data_ptr(), kd.data_ptr(), vt.data_ptr(), out.data_ptr(), lse.data_ptr()
    desc.q_stride_b, desc.q_stride_n, desc.k_stride_b, desc.k_stride_l, desc.vt_stride_b = N * C, C, Lk * C, C, vt.stride(0)
    desc.o_stride_b, desc.o_stride_n = N * C, C
    desc.B, desc.N, desc.H, desc.D, desc.L, desc.Lpad = B, N, heads, d, Lk, vt.shape[-1]
    desc.kv_batch_div, desc.kv2_batch_div, desc.dtype = 1, 1, ops._DT[dtype]
    desc.softmax_scale = 1.0 / math.sqrt(d)
    L.check(L.lib().apad_attention(ctypes.byref(desc), ops._stream()), "apad_attention")
    check(f"attention with lse N={N}")
    lse_check(f"lse N={N}")
    close(out, ref.reshape(B * N, C), TOL[dtype], f"attention with lse N={N} {dtype}")
    assert Npad == N or float(lse[:, N:].abs().max()) == 0.0, "lse pad entries are not 0"
    close(lse[:, :N], (torch.logsumexp(s, -1) * math.log2(math.e)).reshape(B * heads, N), 1e-3, f"lse N={N} {dtype}")
    nan_fill_free(dev)
    out2, lse2 = ops.attention_lse(qd, kd, vt, Lk, heads)
    assert torch.equal(out2.view(B * N, C), out) and torch.equal(lse2.view(B * heads, Npad), lse)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused sub-layers: out= guarded, each at its smallest ragged row count in test_gpu_kernels.py, at that test's bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _xattn_operands(B, N, C, Lt, La, dtype, dev):
    from ap_adapter_amd import ops
    H = 8
    x = E(B, N, C, seed=301)
    g, be = E(C, seed=302, std=0.1, shift=1.0), E(C, seed=303, std=0.1)
    wq, wo, bo = E(C, C, seed=304, std=0.05), E(C, C, seed=305, std=0.05), E(C, seed=306, std=0.3)
    wk, wv, wki, wvi = (E(C, 768, seed=307 + i, std=0.04) for i in range(4))
    et, ea = E(B, Lt, 768, seed=311), E(B, La, 768, seed=312)
    D = lambda t: t.to(dev, dtype)
    k1, k2 = ops.linear(D(et), D(wk)), ops.linear(D(ea), D(wki))
    v1t = torch.zeros(B, H, C // H, ops.round_up(Lt, 32), device=dev, dtype=dtype)
    v2t = torch.zeros(B, H, C // H, ops.round_up(La, 32), device=dev, dtype=dtype)
    ops.linear_vt(D(et), D(wv), B, Lt, H, v1t)
    ops.linear_vt(D(ea), D(wvi), B, La, H, v2t)
    import test_gpu_kernels as K
    dd = lambda t: t.double()
    ref = K._xattn_ref(dd(x), dd(g), dd(be), dd(wq), dd(wo), dd(bo), dd(et), dd(wk), dd(wv), H, None, dd(ea), dd(wki), dd(wvi), 0.55)
    return x, g, be, wq, wo, bo, k1, v1t, k2, v2t, ref


@pytest.mark.parametrize("dtype", DTYPES16)
def test_fused_cross_attention_guarded(dev, dtype):
    from ap_adapter_amd import ops
    B, N, C, Lt, La, H = 1, 33, 256, 8, 64, 8
    x, g, be, wq, wo, bo, k1, v1t, k2, v2t, ref = _xattn_operands(B, N, C, Lt, La, dtype, dev)
    D = lambda t: t.to(dev, dtype)
    ln = (D(g), D(be), 1e-5)
    (wq_p, q_fold), wo_p = ops.xattn_pack_weight(D(wq), ln), ops.xattn_pack_weight(D(wo))
    out, check = guarded(B * N, C, dtype, dev)
    ops.fused_cross_attention(D(x), wq_p, wo_p, D(bo), ops.xattn_pack_kv(k1, v1t, Lt), Lt, H, ln=ln, kv2_packed=ops.xattn_pack_kv(k2, v2t, La),
                              L2=La, scale2=0.55, q_fold=q_fold, out=out.view(B, N, C))
    check("fused_cross_attention")
    close(out, ref.reshape(B * N, C), 1.5 * TOL[dtype], f"fused_cross_attention {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
def test_cross_attention_rows_guarded(dev, dtype):
    from ap_adapter_amd import ops
    B, N, C, Lt, La, H = 1, 33, 384, 8, 64, 8
    x, g, be, wq, wo, bo, k1, v1t, k2, v2t, ref = _xattn_operands(B, N, C, Lt, La, dtype, dev)
    D = lambda t: t.to(dev, dtype)
    out, check = guarded(B * N, C, dtype, dev)
    ops.cross_attention_rows(D(x), ops.xrows_pack_weight(D(wq)), ops.xrows_pack_weight(D(wo)), D(bo), k1, v1t, H, ln=(D(g), D(be), 1e-5),
                             k2=k2, vt2=v2t, scale2=0.55, out=out.view(B, N, C))
    check("cross_attention_rows")
    close(out, ref.reshape(B * N, C), 1.5 * TOL[dtype], f"cross_attention_rows {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("B,N,C", [(2, 33, 256), (3, 130, 384)])
def test_self_attention_fused_guarded(dev, dtype, B, N, C):
    from ap_adapter_amd import ops
    H = 8
    x = E(B, N, C, seed=461, shift=1.5)
    g, be = E(C, seed=462, std=0.1, shift=1.0), E(C, seed=463, std=0.1)
    wq, wk, wv = (E(C, C, seed=464 + i, std=0.06) for i in range(3))
    hs = ln64(x, g, be, 1e-5)
    ref = _attn64(hs @ wq.double().t(), hs @ wk.double().t(), hs @ wv.double().t(), H)[0]
    D = lambda t: t.to(dev, dtype)
    pk, csbb = ops.sattn_pack(D(wq), D(wk), D(wv), (D(g), D(be), 1e-5), H)
    out, check = guarded(B * N, C, dtype, dev)
    ops.self_attention_fused(D(x), pk, csbb, H, 1e-5, out=out.view(B, N, C))
    check("self_attention_fused")
    close(out, ref.reshape(B * N, C), 1.5 * TOL[dtype], f"self_attention_fused N={N} C={C} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("B,N", [(3, 1), (1, 33)])
def test_hs_self_attention_guarded(dev, dtype, B, N):
    """apad_hs_attention (self) + apad_hs_out with both outputs guarded; hs_out allocates the row statistics itself (NaN-filled free
    memory before the launch): finite, and those of the stored rows"""
    from ap_adapter_amd import ops
    import test_gpu_kernels as K
    C, H = 640, 8
    x = E(B, N, C, seed=401)
    g, be = E(C, seed=402, std=0.1, shift=1.0), E(C, seed=403, std=0.1)
    wq, wk, wv = (E(C, C, seed=404 + i, std=0.05) for i in range(3))
    wo, bo = E(C, C, seed=407, std=0.05), E(C, seed=408, std=0.3)
    ref = K._hs_self_ref(*(t.double() for t in (x, g, be, wq, wk, wv, wo, bo)), H)
    D = lambda t: t.to(dev, dtype)
    xd, ln = D(x), (D(g), D(be), 1e-5)
    pk, bb = ops.hs_pack_qkv(D(wq), D(wk), D(wv), ln=ln, q_scale=ops.LOG2E / math.sqrt(C // H))
    wo_p, _ = ops.hs_pack_rows(D(wo))
    o, o_check = guarded(B * N, C, dtype, dev)
    ops.hs_attention(xd, pk, bb, self_attention=True, ln_eps=1e-5, q_prescaled=True, out=o.view(B, N, C))
    o_check("hs_attention (self)")
    out, check = guarded(B * N, C, dtype, dev)
    bod = D(bo)
    nan_fill_free(dev)
    res = ops.hs_out(o.view(B, N, C), wo_p, bod, xd, rowstat=True, out=out.view(B, N, C))
    check("hs_out")
    close(out, ref.reshape(B * N, C), 1.5 * TOL[dtype], f"hs self-attention sub-layer B={B} N={N} {dtype}")
    rs = ops.rowstat_of(res)
    xs = out.double().cpu().view(B * N, 20, 32)
    close(rs.view(B * N, 40), torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).view(B * N, 40), TOL[F32], "hs_out row statistics")


@pytest.mark.parametrize("dtype", DTYPES16)
def test_hs_cross_attention_guarded(dev, dtype):
    from ap_adapter_amd import ops
    B, N, C, Lt, La = 2, 40, 640, 8, 33
    x, g, be, wq, wo, bo, k1, v1t, k2, v2t, ref = _xattn_operands(B, N, C, Lt, La, dtype, dev)
    D = lambda t: t.to(dev, dtype)
    xd, ln = D(x), (D(g), D(be), 1e-5)
    wq_p, qb = ops.hs_pack_rows(D(wq), ln=ln)
    wo_p, _ = ops.hs_pack_rows(D(wo))
    o, o_check = guarded(B * N, C, dtype, dev)
    ops.hs_attention(xd, wq_p, qb, self_attention=False, ln_eps=1e-5, k1=k1, vt1=v1t, k2=k2, vt2=v2t, scale2=0.55, out=o.view(B, N, C))
    o_check("hs_attention (cross)")
    out, check = guarded(B * N, C, dtype, dev)
    ops.hs_out(o.view(B, N, C), wo_p, D(bo), xd, out=out.view(B, N, C))
    check("hs_out")
    close(out, ref.reshape(B * N, C), 1.5 * TOL[dtype], f"hs cross-attention sub-layer {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("B,N", [(1, 1), (3, 16)])
def test_hs_geglu_and_ff2_guarded(dev, dtype, B, N):
    from ap_adapter_amd import ops
    C = 640
    x = E(B, N, C, seed=441, shift=0.5)
    g, be = E(C, seed=442, std=0.1, shift=1.0), E(C, seed=443, std=0.1)
    w1, b1 = E(8 * C, C, seed=444, std=0.05), E(8 * C, seed=445, std=0.2)
    w2, b2 = E(C, 4 * C, seed=453, std=0.03), E(C, seed=454, std=0.3)
    y = ln64(x, g, be, 1e-5) @ w1.double().t() + b1.double()
    a, gt = y.chunk(2, dim=-1)
    D = lambda t: t.to(dev, dtype)
    xd, ln = D(x), (D(g), D(be), 1e-5)
    pk, bb = ops.hs_pack_geglu(D(w1), D(b1), ln=ln)
    h, check = guarded(B * N, 4 * C, dtype, dev)
    ops.hs_geglu(xd, pk, bb, ln_eps=1e-5, out=h.view(B, N, 4 * C))
    check("hs_geglu")
    close(h, (a * gelu64(gt)).reshape(B * N, 4 * C), 1.5 * TOL[dtype], f"hs_geglu B={B} N={N} {dtype}")
    out, check = guarded(B * N, C, dtype, dev)
    ops.hs_ff2(h.view(B, N, 4 * C), ops.hs_pack_ff2(D(w2)), D(b2), xd, out=out.view(B, N, C))
    check("hs_ff2")
    ref = x.double() + h.double().cpu().view(B, N, 4 * C) @ w2.double().t() + b2.double()
    close(out, ref.reshape(B * N, C), TOL[dtype], f"hs_ff2 B={B} N={N} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("M", [37, 257])
def test_geglu_mlp_guarded(dev, dtype, M):
    """apad_geglu_mlp (128-token workgroups) and apad_geglu_mlp_packed (256-token workgroups of 64-token register blocks)"""
    from ap_adapter_amd import ops
    C = 256
    x = E(M, C, seed=156)
    w1, b1 = E(8 * C, C, seed=157, std=0.08), E(8 * C, seed=158, std=0.5)
    w2, b2 = E(C, 4 * C, seed=159, std=0.04), E(C, seed=160, std=0.5)
    g, be = E(C, seed=161, std=0.1, shift=1.0), E(C, seed=162, std=0.1)
    xin = q(ln64(x, g, be, 1e-5).float(), dtype).double()
    a, gate = (xin @ w1.double().t() + b1.double()).chunk(2, dim=-1)
    ref = x.double() + (a * gelu64(gate)) @ w2.double().t() + b2.double()
    D = lambda t: t.to(dev, dtype)
    xd, ln = D(x), (D(g), D(be), 1e-5)
    out, check = guarded(M, C, dtype, dev)
    ops.geglu_mlp(xd, D(w1), D(b1), D(w2), D(b2), ln=ln, out=out)
    check("geglu_mlp")
    close(out, ref, TOL[dtype], f"geglu_mlp M={M} {dtype}")
    wp, bp = ops.mlp_pack(D(w1), D(b1), D(w2))
    out2, check = guarded(M, C, dtype, dev)
    ops.geglu_mlp_packed(xd, wp, bp, D(b2), ln=ln, out=out2)
    check("geglu_mlp_packed")
    close(out2, ref, TOL[dtype], f"geglu_mlp_packed M={M} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("M", [37, 257])
def test_layernorm_geglu_packed_guarded(dev, dtype, M):
    from ap_adapter_amd import ops
    C = 384
    x = E(M, C, seed=656)
    w1, b1 = E(8 * C, C, seed=657, std=0.06), E(8 * C, seed=658, std=0.5)
    g, be = E(C, seed=661, std=0.1, shift=1.0), E(C, seed=662, std=0.1)
    xin = q(ln64(x, g, be, 1e-5).float(), dtype).double()
    a, gate = (xin @ w1.double().t() + b1.double()).chunk(2, dim=-1)
    D = lambda t: t.to(dev, dtype)
    wp, bp = ops.geglu_pack(D(w1), D(b1))
    out, check = guarded(M, 4 * C, dtype, dev)
    ops.layernorm_geglu_packed(D(x), wp, bp, ln=(D(g), D(be), 1e-5), out=out)
    check("layernorm_geglu_packed")
    close(out, a * gelu64(gate), TOL[dtype], f"layernorm_geglu_packed M={M} {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------------
# small ops
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 8, 1000003])
def test_mix3(dev, dtype, n):
    """(a + b + c) * scale: 256-thread grid-stride kernel.  One row of n elements; the guards are 256 rows (>= one workgroup's 256
    elements) for the small counts and one row (n elements) for 1000003 -- whose buffer then starts 2 bytes off a 16-byte boundary"""
    from ap_adapter_amd import ops
    a, b, c = (E(n, seed=91 + i) for i in range(3))
    out, check = guarded(1, n, dtype, dev, guard_rows=1 if n > 256 else 256)
    D = lambda t: t.to(dev, dtype)
    ops.mix3(D(a), D(b), D(c), 0.37, out=out)
    check(f"mix3 n={n}")
    close(out.view(-1, 1), ((a.double() + b.double() + c.double()) * 0.37).view(-1, 1), TOL[dtype], f"mix3 n={n} {dtype}", bm=1 << 16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_rows_and_embedding(dev, dtype):
    """ids -1 and ``rows`` (outside the table: documented to write zeros) give exact zero rows, the others the table's bits; 9 ids: a
    ragged last workgroup of one wave per row"""
    from ap_adapter_amd import ops
    rows, C = 50, 24
    table = E(rows, C, seed=95).to(dev, dtype)
    ids = torch.tensor([0, 49, -1, 7, rows, 3, 3, rows + 100, 48])
    idd = ids.to(dev)
    inside = (ids >= 0) & (ids < rows)
    for fn, shape in ((ops.gather_rows, (9,)), (ops.embedding, (3, 3))):
        nan_fill_free(dev)
        out = fn(table, idd.view(shape)).view(9, C)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out[inside.to(dev)], table[idd[inside.to(dev)]])
        assert bool((out[(~inside).to(dev)].view(torch.int16 if dtype != F32 else torch.int32) == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,Mpad", [(100, 48, 128), (256, 96, 256), (1, 8, 32)])
def test_transpose_pad(dev, dtype, M, C, Mpad):
    """the forward use in clap_audio.py: [M, C] -> [C, Mpad], the pad columns exactly zero"""
    from ap_adapter_amd import ops
    x = E(M, C, seed=96).to(dev, dtype)
    nan_fill_free(dev)
    xt = ops.transpose_pad(x, Mpad)
    assert xt.shape == (C, Mpad) and bool(torch.isfinite(xt).all())
    assert torch.equal(xt[:, :M], x.t())
    assert bool((xt[:, M:].contiguous().view(torch.int16 if dtype != F32 else torch.int32) == 0).all())


def test_window_attention_guarded(dev):
    import clap_audio_models as CM
    from test_gpu_clap_audio import WIN_CASES
    from ap_adapter_amd import ops
    for B, H, W, heads, shift in WIN_CASES:
        C = heads * 24
        qkv = (torch.randn(B, H, W, 3 * C, generator=torch.Generator().manual_seed(H * W + shift)) * 2.2)
        bias = torch.randn(heads, 64, 64, generator=torch.Generator().manual_seed(7 + heads))
        ref = CM.ref_window_attention(qkv, bias, heads, shift)
        out, check = guarded(B * H * W, C, F32, dev)  # (one workgroup per 64-token window)
        ops.window_attention(qkv.view(-1, 3 * C).to(dev), bias.to(dev), B, H, W, heads, shift, out=out)
        what = f"window_attention B={B} {H}x{W} heads={heads} shift={shift}"
        check(what)
        close(out, ref.reshape(B * H * W, C), CM.TOL, what)


def test_clap_mel2img_on_nan_filled_memory(dev):
    import clap_audio_models as CM
    from ap_adapter_amd import ops
    T, Fb, S = 251, 16, 64
    R = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed))
    x = CM.features((2, 1, T, Fb), seed=T)
    w, b, mean, var = 1 + 0.1 * R(Fb, seed=1), 0.2 * R(Fb, seed=2), 0.3 * R(Fb, seed=3), 0.5 + torch.rand(Fb, generator=torch.Generator().manual_seed(4))
    ref = CM.ref_mel2img(x, w, b, mean, var, 1e-5, S)
    args = [t.to(dev) for t in (x, w, b, mean, var)]
    nan_fill_free(dev)
    out = ops.clap_mel2img(*args, 1e-5, S)
    close(out, ref, CM.TOL, "clap_mel2img")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_sample_on_nan_filled_memory(dev, dtype):
    from ap_adapter_amd import ops
    rows, Lc = 37, 8
    m, n = E(rows, 2 * Lc, seed=97, std=3.0), E(rows, Lc, seed=98)
    m[0, Lc:], m[1, Lc:] = 50.0, -50.0  # clamped to 20 / -30
    ref = (m[:, :Lc].double() + torch.exp(0.5 * m[:, Lc:].double().clamp(-30, 20)) * n.double()) * 0.41
    md, nd = m.to(dev, dtype), n.to(dev, dtype)
    nan_fill_free(dev)
    out = ops.gaussian_sample(md, nd, 0.41)
    close(out, ref, TOL[dtype], f"gaussian_sample {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_audiomae_pool_on_nan_filled_memory(dev, dtype):
    from ap_adapter_amd import ops
    from oracle.audiomae import pool
    rep = E(2, 513, 768, seed=43)
    ref = pool(rep.double(), 2, 2)
    rd = rep.to(dev, dtype)
    nan_fill_free(dev)
    out = ops.audiomae_pool(rd, 2, 2)
    assert out.shape == ref.shape
    close(out.view(-1, 768), ref.reshape(-1, 768), TOL[dtype], f"audiomae_pool {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_timestep_embedding_on_nan_filled_memory(dev, dtype):
    """fp32 at the bound test_gpu_kernels.py::test_timestep_embedding states for it (1e-4: one ulp of a frequency at t ~ 1000)"""
    from ap_adapter_amd import ops
    from oracle.blocks import timestep_embedding
    t = torch.tensor([996.0, 991.0, 501.0, 1.0, 0.0])
    ref = timestep_embedding(t, 128, True, 0.0)
    td = t.to(dev)
    nan_fill_free(dev)
    out = ops.timestep_embedding(td, 128, True, 0.0, dtype)
    close(out, ref, 1e-4 if dtype == F32 else TOL[dtype], f"timestep_embedding {dtype}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_patch_embed_on_nan_filled_memory(dev, mode):
    from ap_adapter_amd import ops
    dtype, prec = mode
    mel = E(2, 32, 48, seed=20, std=0.5)
    w, b = E(768, 1, 16, 16, seed=21, std=0.05), E(768, seed=22, std=0.1)
    ref = F.conv2d(mel.double().unsqueeze(1), w.double(), b.double(), stride=16).flatten(2).transpose(1, 2)
    md, wd, bd = mel.to(dev), w.reshape(768, 256).to(dev, dtype), b.to(dev, dtype)
    with precision(prec):
        nan_fill_free(dev)
        out = ops.patch_embed(md, wd, bd, dtype)
    close(out.view(-1, 768), ref.reshape(-1, 768), TOL[dtype], f"patch_embed {dtype} {prec}")

"""-m gpu: every distinct backward launch of the cfg-5 training micro-step, alone, at its real shape, against fp64 torch autograd.

The step is bench.py::train_measure's: the full-geometry UNet in bf16, batch 4, latent 250 x 16, La = 32 (8 GPT-2 + 32 audio
tokens at the IP sites), 16 T5 tokens with the last 4 masked on odd rows.  CENSUS below lists its backward launches;
test_backward_census_matches_the_step records them from one micro-step, so the table cannot go stale.  Every entry is then run
alone in bf16, f16 and fp32.

Operands are drawn in fp32, rounded to bf16 and flushed to zero below 2^-14 (util.exact_operand): exact in all three types, so
only the kernels' arithmetic differs from the fp64 reference.  Before each measured call the free blocks of the caching allocator
are filled with NaN (util.nan_fill_free): an output element, pad column or delta entry a kernel fails to write reads as NaN.

Bounds (error = max |out - ref|):
  global     relative to max|ref| of the tensor: TOL[dtype], 1.5 x TOL for attention gradients (as tests/test_gpu_train.py).
  per block  relative to the block's own max|ref|: BLOCK_TOL[dtype] = 1.5e-2 / 2e-3 / 5e-6 (bf16 / f16 / fp32).  Block = (sample,
             head) for attention, a row for LayerNorm, GEGLU, linear dgrad and dW, a (sample, group) for GroupNorm, a (sample, row of
             the input) for the convolution dgrad.  A wrong tail tile, head, group or pad row cannot hide under the global maximum.
             Measured worst over the table: 9.3e-3 (bf16, LayerNorm 4000 x 256), 1.13e-3 (f16, LayerNorm 1008 x 384), 2.6e-6
             (fp32, linear dgrad 256 x 5120 -> 640).
  exact      every output finite; dk and dv of masked keys 0; need_dkv=False leaves dq bit-equal; packed=True bit-equal to the
             unpacked call; attention_lse's pad entries 0.
  lse        attention_lse (base 2) within 1e-5 relative of fp64 logsumexp / ln 2.
  off-centre LN / GN inputs whose rows / groups sit at twice the largest |mean| / std the census measured for that launch (OFF in
             the table): the same bounds as centred inputs.
Run with -s to see every measured value."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from util import TOL, block_rel_err, exact_operand, nan_fill_free

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}

# ---------------------------------------------------------------------------------------------------------------------
# Census of the cfg-5 micro-step's backward launches (one row per distinct launch; the count is how often the step makes it).
# Levels: 4000 / 1000 / 252 / 64 tokens at C = 128 / 256 / 384 / 640, 8 heads.  OFF: the bound on the largest |mean| / std of a
# row (LayerNorm) or a (sample, group) (GroupNorm) of the launch's x that the census measured (rounded up).
# ---------------------------------------------------------------------------------------------------------------------
ATTENTION_BWD = [  # B, N, L, heads, d, packed, need_dkv, acc_dq, dout_scale, key_bias : count
    ((4, 1000, 1000, 8, 32, True, True, False, 1.0, False), 55),
    ((4, 1000, 16, 8, 32, False, False, False, 1.0, True), 10),
    ((4, 1000, 32, 8, 32, False, True, True, 0.5, False), 10),
    ((4, 1000, 8, 8, 32, False, False, False, 1.0, False), 10),
    ((4, 252, 16, 8, 48, False, False, False, 1.0, True), 10),
    ((4, 252, 252, 8, 48, True, True, False, 1.0, False), 60),
    ((4, 252, 32, 8, 48, False, True, True, 0.5, False), 10),
    ((4, 252, 8, 8, 48, False, False, False, 1.0, False), 10),
    ((4, 64, 16, 8, 80, False, False, False, 1.0, True), 12),
    ((4, 64, 32, 8, 80, False, True, True, 0.5, False), 12),
    ((4, 64, 64, 8, 80, True, True, False, 1.0, False), 72),
    ((4, 64, 8, 8, 80, False, False, False, 1.0, False), 12),
]
LAYER_NORM_BWD = [  # M, C, eps, dres, OFF : count
    ((1008, 384, 1e-05, True, 0.3), 120),  # measured |mean|/std 0.212
    ((256, 640, 1e-05, True, 0.2), 144),  # measured |mean|/std 0.162
    ((4000, 256, 1e-05, True, 0.3), 112),  # measured |mean|/std 0.265
]
GROUP_NORM_BWD = [  # B, HW, C, G, eps, silu, OFF : count
    ((4, 1000, 256, 32, 1e-05, True, 0.6), 5),  # measured |mean|/std 0.541
    ((4, 1000, 256, 32, 1e-06, False, 0.7), 18),  # measured |mean|/std 0.570
    ((4, 1000, 384, 32, 1e-05, True, 0.4), 1),  # measured |mean|/std 0.315
    ((4, 1000, 512, 32, 1e-05, True, 0.4), 1),  # measured |mean|/std 0.332
    ((4, 1000, 640, 32, 1e-05, True, 0.3), 1),  # measured |mean|/std 0.272
    ((4, 252, 1024, 32, 1e-05, True, 0.3), 1),  # measured |mean|/std 0.239
    ((4, 252, 256, 32, 1e-05, True, 0.6), 1),  # measured |mean|/std 0.506
    ((4, 252, 384, 32, 1e-05, True, 0.6), 6),  # measured |mean|/std 0.469
    ((4, 252, 384, 32, 1e-06, False, 0.7), 20),  # measured |mean|/std 0.596
    ((4, 252, 640, 32, 1e-05, True, 0.4), 1),  # measured |mean|/std 0.338
    ((4, 252, 768, 32, 1e-05, True, 0.3), 1),  # measured |mean|/std 0.238
    ((4, 4000, 128, 32, 1e-05, True, 0.8), 4),  # measured |mean|/std 0.653
    ((4, 4000, 256, 32, 1e-05, True, 0.6), 2),  # measured |mean|/std 0.455
    ((4, 4000, 384, 32, 1e-05, True, 0.6), 1),  # measured |mean|/std 0.462
    ((4, 64, 1024, 32, 1e-05, True, 0.3), 1),  # measured |mean|/std 0.238
    ((4, 64, 1280, 32, 1e-05, True, 0.4), 2),  # measured |mean|/std 0.276
    ((4, 64, 384, 32, 1e-05, True, 0.5), 1),  # measured |mean|/std 0.379
    ((4, 64, 640, 32, 1e-05, True, 0.6), 10),  # measured |mean|/std 0.485
    ((4, 64, 640, 32, 1e-06, False, 0.6), 24),  # measured |mean|/std 0.455
]
GEGLU_BWD = [  # M, N : count
    ((1008, 1536), 40),
    ((256, 2560), 48),
    ((4000, 1024), 38),
]
WEIGHT_GRAD = [  # M, N, K, fp32, acc : count
    ((128, 256, 768, True, True), 20),
    ((128, 384, 768, True, True), 20),
    ((128, 640, 768, True, True), 24),
]
LINEAR_DGRAD = [  # M, N, K (dx [M, K] = dy [M, N] . W [N, K]) : count
    ((1008, 3072, 384), 40),
    ((1008, 384, 1024), 1),
    ((1008, 384, 1536), 40),
    ((1008, 384, 256), 1),
    ((1008, 384, 384), 140),
    ((1008, 384, 640), 1),
    ((1008, 384, 768), 1),
    ((16000, 128, 256), 2),
    ((16000, 128, 384), 1),
    ((256, 5120, 640), 48),
    ((256, 640, 1024), 1),
    ((256, 640, 1280), 2),
    ((256, 640, 2560), 48),
    ((256, 640, 384), 1),
    ((256, 640, 640), 168),
    ((4000, 2048, 256), 38),
    ((4000, 256, 1024), 38),
    ((4000, 256, 256), 131),
    ((4000, 256, 384), 1),
    ((4000, 256, 512), 1),
    ((4000, 256, 640), 1),
]
CONV_DGRAD = [  # B, H, W, Cin, Cout, mode ("s1", "s2" or the upsampled size (Hup, Wup)) : count
    ((4, 125, 8, 256, 256, 's1'), 5),
    ((4, 125, 8, 256, 256, 's2'), 1),
    ((4, 125, 8, 256, 256, (250, 16)), 1),
    ((4, 125, 8, 384, 256, 's1'), 1),
    ((4, 125, 8, 512, 256, 's1'), 1),
    ((4, 125, 8, 640, 256, 's1'), 1),
    ((4, 250, 16, 128, 128, 's1'), 3),
    ((4, 250, 16, 128, 8, 's1'), 1),
    ((4, 250, 16, 256, 128, 's1'), 2),
    ((4, 250, 16, 384, 128, 's1'), 1),
    ((4, 32, 2, 1024, 640, 's1'), 1),
    ((4, 32, 2, 1280, 640, 's1'), 2),
    ((4, 32, 2, 384, 640, 's1'), 1),
    ((4, 32, 2, 640, 640, 's1'), 10),
    ((4, 32, 2, 640, 640, (63, 4)), 1),
    ((4, 63, 4, 1024, 384, 's1'), 1),
    ((4, 63, 4, 256, 384, 's1'), 1),
    ((4, 63, 4, 384, 384, 's1'), 6),
    ((4, 63, 4, 384, 384, 's2'), 1),
    ((4, 63, 4, 384, 384, (125, 8)), 1),
    ((4, 63, 4, 640, 384, 's1'), 1),
    ((4, 63, 4, 768, 384, 's1'), 1),
]
CENSUS = {"attention_bwd": ATTENTION_BWD, "layer_norm_bwd": LAYER_NORM_BWD, "group_norm_bwd": GROUP_NORM_BWD, "geglu_bwd": GEGLU_BWD,
          "weight_grad": WEIGHT_GRAD, "linear_dgrad": LINEAR_DGRAD, "conv_dgrad": CONV_DGRAD}
_OFF_OPS = ("layer_norm_bwd", "group_norm_bwd")  # entries end with OFF (not part of the launch's identity)


def _key(op, entry):
    return tuple(entry[:-1]) if op in _OFF_OPS else tuple(entry)


# per-block bound (module docstring), set above the worst case measured over the whole table in each type: bf16 9.3e-3, f16 1.13e-3,
# fp32 2.6e-6 (attention alone: 7.6e-3 / 9.1e-4 / 1.2e-6)
BLOCK_TOL = {torch.bfloat16: 1.5e-2, torch.float16: 2e-3, torch.float32: 5e-6}

_WORST = {}  # (op, dtype, what) -> (worst value, entry): printed at the end of the module


def _note(op, dtype, what, val, entry):
    k = (op, DT_NAME[dtype], what)
    if k not in _WORST or val > _WORST[k][0]:
        _WORST[k] = (val, entry)


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    if _WORST:
        print("\n[backward shapes] worst measured value per (op, dtype, bound):")
        for (op, dt, what), (v, e) in sorted(_WORST.items()):
            print(f"  {op:15s} {dt:4s} {what:22s} {v:.3e}  at {e}")


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _warm_then_fill(dev, run):
    """run once (so the allocator holds blocks of the launch's sizes), drop the outputs, fill the free blocks with NaN, run again"""
    out = run()
    del out
    nan_fill_free(dev)
    return run()


def _check(op, dtype, entry, name, got, want, nblocks, tol_mul=1.0):
    """finite + global (tol_mul x TOL) + per-block (BLOCK_TOL) bounds of one output; returns (global, per-block) error"""
    got = got.detach().double().cpu()
    bad = (~torch.isfinite(got)).nonzero()
    assert bad.numel() == 0, f"{op} {entry} {DT_NAME[dtype]} {name}: {bad.shape[0]} non-finite outputs, first at {bad[:4].tolist()}"
    g = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    b, bi = block_rel_err(got, want, nblocks)
    print(f"  {op} {entry} {DT_NAME[dtype]} {name}: global {g:.2e}  worst block {b:.2e} (#{bi} of {nblocks})")
    _note(op, dtype, name + " global", g, entry)
    _note(op, dtype, name + " block", b, entry)
    assert g < tol_mul * TOL[dtype], f"{op} {entry} {DT_NAME[dtype]} {name}: global {g:.3e}"
    assert b < BLOCK_TOL[dtype], f"{op} {entry} {DT_NAME[dtype]} {name}: block #{bi} of {nblocks} at {b:.3e}"
    return g, b


def test_nan_fill_reaches_reused_memory(dev):
    """the premise of the 'every output finite' checks: a buffer the allocator hands out again after nan_fill_free reads NaN"""
    for n in (7, 4096, 3 << 20):  # (small and large allocator pools)
        t = torch.zeros(n, dtype=torch.float32, device=dev)  # (the widest of the three: every later request fits its block)
        del t
        for dt in DTYPES:
            nan_fill_free(dev)  # (again per check: the previous check's own result tensor reused filled memory)
            assert bool(torch.isnan(torch.empty(n, dtype=dt, device=dev)).all()), (n, dt)


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------
def _row_offset(x2d):
    r = x2d.double()
    return float((r.mean(1).abs() / r.std(1, unbiased=False).clamp_min(1e-30)).max())


def record_census(dev, dtype=torch.bfloat16):
    """One AdapterTrainer.micro_step of bench.py::train_measure's geometry with every backward entry point wrapped.  Returns
    {op: {launch key: [count, largest |mean|/std of x (LN / GN), ...]}}."""
    import ap_adapter_amd as A
    from ap_adapter_amd import autograd as AG
    from ap_adapter_amd import ops
    from ap_adapter_amd.synthetic import synthetic_inputs
    from util import full_unet
    rec = {op: {} for op in CENSUS}

    def note(op, key, off=None):
        e = rec[op].setdefault(key, [0, 0.0])
        e[0] += 1
        if off is not None:
            e[1] = max(e[1], off)

    saved = []

    def patch(owner, name, new):
        saved.append((owner, name, owner.__dict__[name]))
        setattr(owner, name, new)

    o_attn, o_ln, o_gn, o_geglu, o_wg = ops.attention_bwd, ops.layer_norm_bwd, ops.group_norm_bwd, ops.geglu_bwd, ops.weight_grad

    def attention_bwd(q, k, v, out, dout, lse, heads, key_bias=None, dout_scale=1.0, need_dkv=True, dq=None, packed=False):
        B, N, C_ = q.shape
        note("attention_bwd", (B, N, k.shape[1], heads, C_ // heads, bool(packed), bool(need_dkv), dq is not None, float(dout_scale),
                               key_bias is not None))
        return o_attn(q, k, v, out, dout, lse, heads, key_bias=key_bias, dout_scale=dout_scale, need_dkv=need_dkv, dq=dq, packed=packed)

    def layer_norm_bwd(x, gamma, dy, eps, dres=None):
        C_ = x.shape[-1]
        note("layer_norm_bwd", (x.numel() // C_, C_, float(eps), dres is not None), _row_offset(x.reshape(-1, C_)))
        return o_ln(x, gamma, dy, eps, dres=dres)

    def group_norm_bwd(x, gamma, beta, dy, groups, eps, silu):
        B, HW, C_ = x.shape
        xg = x.reshape(B, HW, groups, C_ // groups).permute(0, 2, 1, 3).reshape(B * groups, -1)
        note("group_norm_bwd", (B, HW, C_, groups, float(eps), bool(silu)), _row_offset(xg))
        return o_gn(x, gamma, beta, dy, groups, eps, silu)

    def geglu_bwd(proj, dh):
        note("geglu_bwd", (proj.numel() // proj.shape[-1], proj.shape[-1] // 2))
        return o_geglu(proj, dh)

    def weight_grad(dy, x, fp32=False, acc=None):
        note("weight_grad", (dy.shape[0], dy.shape[1], x.shape[-1], bool(fp32), acc is not None))
        return o_wg(dy, x, fp32=fp32, acc=acc)

    conv_bwd, lin_bwd = AG._Conv3x3.backward, AG._Linear.backward

    def conv_backward(ctx, dy):
        if ctx.needs_input_grad[0]:
            (w,) = ctx.saved_tensors
            B, H, W, stride, up, _ = ctx.geom
            note("conv_dgrad", (B, H, W, w.shape[1], w.shape[0], "s2" if stride == 2 else (tuple(up) if up is not None else "s1")))
        return conv_bwd(ctx, dy)

    def linear_backward(ctx, dy):
        if ctx.needs_input_grad[0]:
            w = ctx.saved_tensors[1]
            note("linear_dgrad", (dy.numel() // dy.shape[-1], w.shape[0], w.reshape(w.shape[0], -1).shape[1]))
        return lin_bwd(ctx, dy)

    B, La = 4, 32
    u = full_unet(0.5).to(dtype)  # (bench.py installs the adapter at scale 0.5)
    inp = synthetic_inputs(B, La)
    ehs = A.AudioLDM2Pipeline(u).assemble_condition(inp["generated_prompt_embeds"], inp["audio_tokens"], inp["uncond_audio_tokens"], dtype)[B:]
    ehs1 = inp["prompt_embeds"].to(dtype)[B:]
    m1 = inp["attention_mask"].float()[B:]  # (rows 1 and 3: the last 4 T5 tokens masked)
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(B, 8, 250, 16, generator=g)
    t = torch.tensor([437, 12, 880, 651])
    u = u.to(dev)
    tr = A.AdapterTrainer(u)
    noisy = A.add_noise(inp["latents"].to(dev), noise.to(dev), t.to(dev), tr.alphas_cumprod)
    for owner, name, new in ((ops, "attention_bwd", attention_bwd), (ops, "layer_norm_bwd", layer_norm_bwd),
                             (ops, "group_norm_bwd", group_norm_bwd), (ops, "geglu_bwd", geglu_bwd), (ops, "weight_grad", weight_grad),
                             (AG._Conv3x3, "backward", staticmethod(conv_backward)), (AG._Linear, "backward", staticmethod(linear_backward))):
        patch(owner, name, new)
    try:
        tr.micro_step(noisy, t.to(dev), ehs.to(dev), ehs1.to(dev), m1.to(dev), noise.to(dev))
        torch.cuda.synchronize(dev)
    finally:
        for owner, name, old in reversed(saved):
            setattr(owner, name, old)
    return rec


def format_census(rec):
    """the recorded launches in the table's literal form (OFF: the measured offset, rounded up)"""
    lines = []
    for op, entries in rec.items():
        lines.append(f"{op}:")
        for key, (n, off) in sorted(entries.items(), key=lambda kv: repr(kv[0])):
            extra = f", {math.ceil(off * 1.1 * 10) / 10}" if op in _OFF_OPS else ""
            note = f"  # measured |mean|/std {off:.3f}" if op in _OFF_OPS else ""
            lines.append(f"    (({', '.join(repr(v) for v in key)}{extra}), {n}),{note}")
    return "\n".join(lines)


def test_backward_census_matches_the_step(dev):
    """the table above is what the step launches: no launch missing, none extra, no shape changed; and no LN / GN launch of the
    step sees rows / groups further off centre than the OFF the table gives it (the off-centre tests run at twice that)"""
    rec = record_census(dev)
    print("\n[census] recorded backward launches of one cfg-5 micro-step:\n" + format_census(rec))
    for op, table in CENSUS.items():
        want = {_key(op, e[0]): e[1] for e in table}
        got = {k: v[0] for k, v in rec[op].items()}
        assert set(got) == set(want), (f"{op}: missing from the step {sorted(set(want) - set(got), key=repr)}; "
                                       f"not in the table {sorted(set(got) - set(want), key=repr)}")
        assert got == want, f"{op}: launch counts differ: {got} vs table {want}"
        if op in _OFF_OPS:
            for e, _n in table:
                assert rec[op][_key(op, e)][1] <= e[-1], f"{op} {e}: x measured at |mean|/std {rec[op][_key(op, e)][1]:.3f} > OFF {e[-1]}"


def _entries(op):
    return [pytest.param(e, id="-".join(str(v).replace(" ", "") for v in e)) for e, _n in CENSUS[op]]


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _sdpa(q, k, v, heads, bias=None):
    B, N, C_ = q.shape
    sp = lambda t: t.reshape(B, t.shape[1], heads, C_ // heads).transpose(1, 2)
    m = None if bias is None else bias[:, None, None, :]
    o = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=m)
    return o.transpose(1, 2).reshape(B, N, C_)


def _t5_bias(B, L):
    """the step's T5 mask: the last 4 keys of odd rows dropped (synthetic_inputs), as the UNet's additive bias"""
    kb = torch.zeros(B, L)
    kb[1::2, -4:] = -10000.0
    return kb


def _attn_operands(B, N, L, heads, d, key_bias):
    C_ = heads * d
    s = _seed("attn", B, N, L, heads, d)
    q, k, v, do = (exact_operand(B, n, C_, seed=s + i) for i, n in enumerate((N, L, L, N)))
    return q, k, v, do, (_t5_bias(B, L) if key_bias else None)


def _attn_ref(B, N, L, heads, d, key_bias):
    """fp64 (dq, dk, dv) of one unscaled segment, and its base-2 log-sum-exp [B, heads, N]"""
    def make():
        q, k, v, do, kb = _attn_operands(B, N, L, heads, d, key_bias)
        ql, kl, vl = (t.double().requires_grad_(True) for t in (q, k, v))
        kb64 = None if kb is None else kb.double()
        _sdpa(ql, kl, vl, heads, kb64).backward(do.double())
        C_ = heads * d
        sc = torch.einsum("bnhd,blhd->bhnl", q.double().reshape(B, N, heads, d), k.double().reshape(B, L, heads, d)) / math.sqrt(d)
        if kb64 is not None:
            sc = sc + kb64[:, None, None, :]
        lse2 = torch.logsumexp(sc, -1) / math.log(2.0)
        return ql.grad, kl.grad, vl.grad, lse2
    return _cached(("attn", B, N, L, heads, d, key_bias), make)


def _run_attention_bwd(dev, dtype, entry, *, need_dkv=None, packed=None, dq0=None):
    """the entry's launch on device operands (forward by apad_attention, as in the step): returns (dq, dk, dv, lse)"""
    from ap_adapter_amd import ops
    B, N, L, heads, d, pk, nd, acc, s, kb = entry
    need_dkv = nd if need_dkv is None else need_dkv
    packed = pk if packed is None else packed
    q, k, v, do, bias = (None if t is None else t.to(dev, dtype) for t in _attn_operands(B, N, L, heads, d, kb))
    if bias is not None:
        bias = bias.to(dev, torch.float32)
    vt = ops.head_transpose(v, heads)
    nan_fill_free(dev)
    o, lse = ops.attention_lse(q, k, vt, L, heads, key_bias=bias)

    def run():
        dq = None if dq0 is None else dq0.to(dev, dtype).clone()
        return ops.attention_bwd(q, k, v, o, do, lse, heads, key_bias=bias, dout_scale=s, need_dkv=need_dkv, dq=dq, packed=packed)
    dq, dk, dv = _warm_then_fill(dev, run)
    torch.cuda.synchronize(dev)
    return dq, dk, dv, lse


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("entry", _entries("attention_bwd"))
def test_attention_bwd_entry(dev, dtype, entry):
    """dq (accumulated into a prefilled dq where the step accumulates), dk, dv, with the entry's dout_scale and key bias; the
    forward's log-sum-exp; dq bit-equal with and without the dk / dv pass; packed bit-equal to unpacked; masked keys exactly 0"""
    B, N, L, heads, d, packed, need_dkv, acc, s, kb = entry
    C_ = heads * d
    dq_r, dk_r, dv_r, lse_r = _attn_ref(B, N, L, heads, d, kb)
    dq0 = exact_operand(B, N, C_, seed=_seed("dq0", entry), std=0.1) if acc else None
    dq, dk, dv, lse = _run_attention_bwd(dev, dtype, entry, dq0=dq0)
    nb = B * heads
    per_head = lambda t: t.reshape(B, -1, heads, d).transpose(1, 2)  # blocks (b, head)
    want_dq = s * dq_r + (0 if dq0 is None else dq0.double())
    _check("attention_bwd", dtype, entry, "dq", per_head(dq), per_head(want_dq), nb, 1.5)
    if need_dkv:
        _check("attention_bwd", dtype, entry, "dk", per_head(dk), per_head(s * dk_r), nb, 1.5)
        _check("attention_bwd", dtype, entry, "dv", per_head(dv), per_head(s * dv_r), nb, 1.5)
    else:
        assert dk is None and dv is None
    # the forward's statistics: base-2 log-sum-exp, pad entries written as 0
    lse = lse.cpu()
    Npad = lse.shape[-1]
    assert torch.isfinite(lse).all() and bool((lse[..., N:] == 0).all()), "attention_lse: pad entries not 0"
    lrel = float(((lse[..., :N].double() - lse_r).abs() / lse_r.abs().clamp_min(1.0)).max())
    print(f"  attention_lse {entry[:5]} {DT_NAME[dtype]}: rel err {lrel:.2e} (Npad {Npad})")
    _note("attention_lse", dtype, "rel", lrel, entry[:5])
    assert lrel < 1e-5
    # dq does not depend on whether the dk / dv pass runs (the dq pass writes delta for it)
    dq2, dk2, dv2, _ = _run_attention_bwd(dev, dtype, entry, need_dkv=not need_dkv, dq0=dq0)
    assert torch.equal(dq2, dq), "dq changes with need_dkv"
    dkm, dvm = (dk, dv) if need_dkv else (dk2, dv2)
    if kb:  # masked keys receive exactly nothing
        m = _t5_bias(B, L) < 0
        assert bool((dkm.cpu()[m] == 0).all()) and bool((dvm.cpu()[m] == 0).all()), "masked keys got a gradient"
        assert bool((dkm.cpu()[~m].abs().amax(-1) > 0).all()), "an unmasked key got no gradient"
    if packed:
        dq3, dk3, dv3, _ = _run_attention_bwd(dev, dtype, entry, packed=False, dq0=dq0)
        assert torch.equal(dq3, dq) and torch.equal(dk3, dk) and torch.equal(dv3, dv), "packed != unpacked"


def _ip_pairs():
    """(text entry, audio entry) of every IP site: the audio segment accumulates into the text segment's dq"""
    out = []
    for a, _n in ATTENTION_BWD:
        if a[7]:
            t = [e for e, _m in ATTENTION_BWD if e[:2] == a[:2] and e[3:5] == a[3:5] and not (e[6] or e[7] or e[9])]
            assert len(t) == 1, (a, t)
            out.append(pytest.param(t[0], a, id=f"{a[0]}-{a[1]}-{a[4]}"))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("text,audio", _ip_pairs())
def test_ip_pair_accumulated_dq(dev, dtype, text, audio):
    """the decoupled cross-attention's two launches in the step's order (autograd._IPAttention.backward): dq of the text segment,
    then the audio segment with dout_scale = ap_scale accumulating into it; against fp64 dq_text + s dq_audio, s dk_audio, s dv_audio"""
    from ap_adapter_amd import ops
    B, N, Lt, heads, d = text[:5]
    La, s = audio[2], audio[8]
    q, kt, vt_, do, _ = (None if t is None else t.to(dev, dtype) for t in _attn_operands(B, N, Lt, heads, d, False))
    _, ka, va, _, _ = (None if t is None else t.to(dev, dtype) for t in _attn_operands(B, N, La, heads, d, False))
    ql, ktl, vtl, kal, val = (t.cpu().double().requires_grad_(True) for t in (q, kt, vt_, ka, va))
    (_sdpa(ql, ktl, vtl, heads) + s * _sdpa(ql, kal, val, heads)).backward(do.cpu().double())
    o_t, lse_t = ops.attention_lse(q, kt, ops.head_transpose(vt_, heads), Lt, heads)
    o_a, lse_a = ops.attention_lse(q, ka, ops.head_transpose(va, heads), La, heads)

    def run():
        dq, _, _ = ops.attention_bwd(q, kt, vt_, o_t, do, lse_t, heads, need_dkv=text[6])
        _, dk, dv = ops.attention_bwd(q, ka, va, o_a, do, lse_a, heads, dout_scale=s, need_dkv=audio[6], dq=dq)
        return dq, dk, dv
    dq, dk, dv = _warm_then_fill(dev, run)
    per_head = lambda t: t.reshape(B, -1, heads, d).transpose(1, 2)
    for name, got, want in (("dq", dq, ql.grad), ("dk_ip", dk, kal.grad), ("dv_ip", dv, val.grad)):
        _check("ip_pair", dtype, (B, N, Lt, La, heads, d, s), name, per_head(got), per_head(want), B * heads, 1.5)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm / GroupNorm: centred and off-centre inputs
# ---------------------------------------------------------------------------------------------------------------------
def _shifts(n, off, seed):
    """n shifts in [-off, off] with both ends attained, in a random order (so the extreme rows are not the first or last)"""
    if off == 0:
        return torch.zeros(n)
    v = torch.linspace(-off, off, n)
    return v[torch.randperm(n, generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("centre", ["centred", "off"])
@pytest.mark.parametrize("entry", _entries("layer_norm_bwd"))
def test_layer_norm_bwd_entry(dev, dtype, centre, entry):
    """dx of LayerNorm (+ the residual gradient the step fuses into the launch) per row; 'off': rows at up to twice the census'
    largest |mean| / std"""
    from ap_adapter_amd import ops
    M, C_, eps, dres, off = entry
    shift_to = 2 * off if centre == "off" else 0.0
    s = _seed("ln", M, C_)
    x = exact_operand(M, C_, seed=s, shift=_shifts(M, shift_to, s)[:, None])
    g, b = exact_operand(C_, seed=s + 1, std=0.1) + 1, exact_operand(C_, seed=s + 2, std=0.1)
    dy = exact_operand(M, C_, seed=s + 3)
    r = exact_operand(M, C_, seed=s + 4) if dres else None

    def make():
        xl = x.double().requires_grad_(True)
        F.layer_norm(xl, (C_,), g.double(), b.double(), eps).backward(dy.double())
        return xl.grad + (0 if r is None else r.double())
    want = _cached(("ln", entry, centre), make)
    print(f"  layer_norm_bwd {entry} {centre}: x at |mean|/std up to {_row_offset(x):.2f}")
    D = lambda t: None if t is None else t.to(dev, dtype)
    xd, gd, dyd, rd = D(x), D(g), D(dy), D(r)
    got = _warm_then_fill(dev, lambda: ops.layer_norm_bwd(xd, gd, dyd, eps, dres=rd))
    _check("layer_norm_bwd" + ("" if centre == "centred" else "/off"), dtype, entry, "dx", got, want, M)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("centre", ["centred", "off"])
@pytest.mark.parametrize("entry", _entries("group_norm_bwd"))
def test_group_norm_bwd_entry(dev, dtype, centre, entry):
    """dx of GroupNorm (+ SiLU) per (sample, group); 'off': groups at up to twice the census' largest |mean| / std"""
    from ap_adapter_amd import ops
    B, HW, C_, G, eps, silu, off = entry
    shift_to = 2 * off if centre == "off" else 0.0
    s = _seed("gn", B, HW, C_, G)
    sh = _shifts(B * G, shift_to, s).reshape(B, 1, G, 1).expand(B, 1, G, C_ // G).reshape(B, 1, C_)
    x = exact_operand(B, HW, C_, seed=s, shift=sh)
    g, b = exact_operand(C_, seed=s + 1, std=0.1) + 1, exact_operand(C_, seed=s + 2, std=0.1)
    dy = exact_operand(B, HW, C_, seed=s + 3)

    def make():
        xl = x.double().requires_grad_(True)
        y = F.group_norm(xl.transpose(1, 2), G, g.double(), b.double(), eps)
        (F.silu(y) if silu else y).transpose(1, 2).backward(dy.double())
        return xl.grad
    want = _cached(("gn", entry, centre), make)
    xg = x.reshape(B, HW, G, C_ // G).permute(0, 2, 1, 3).reshape(B * G, -1)
    print(f"  group_norm_bwd {entry} {centre}: x at |mean|/std up to {_row_offset(xg):.2f}")
    D = lambda t: t.to(dev, dtype)
    xd, gd, bd, dyd = D(x), D(g), D(b), D(dy)
    got = _warm_then_fill(dev, lambda: ops.group_norm_bwd(xd, gd, bd, dyd, G, eps, silu))
    blocks = lambda t: t.reshape(B, HW, G, C_ // G).transpose(1, 2)  # (b, group)
    _check("group_norm_bwd" + ("" if centre == "centred" else "/off"), dtype, entry, "dx", blocks(got), blocks(want), B * G)


# ---------------------------------------------------------------------------------------------------------------------
# GEGLU, dW, linear and convolution dgrad
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("entry", _entries("geglu_bwd"))
def test_geglu_bwd_entry(dev, dtype, entry):
    from ap_adapter_amd import ops
    M, N = entry
    s = _seed("geglu", M, N)
    proj, dh = exact_operand(M, 2 * N, seed=s), exact_operand(M, N, seed=s + 1)

    def make():
        pl = proj.double().requires_grad_(True)
        a, gt = pl.chunk(2, dim=-1)
        (a * F.gelu(gt)).backward(dh.double())
        return pl.grad
    want = _cached(("geglu", entry), make)
    pd, dhd = proj.to(dev, dtype), dh.to(dev, dtype)
    got = _warm_then_fill(dev, lambda: ops.geglu_bwd(pd, dhd))
    _check("geglu_bwd", dtype, entry, "dproj", got, want, M)


def _wgrad_case(dev, dtype, M, N, K, fp32, acc, seed):
    """dW = dy^T x through ops.weight_grad, called twice onto a prefilled fp32 accumulator when ``acc`` (the step's
    AdapterTrainer grad sink); returns (got, fp64 reference)"""
    from ap_adapter_amd import ops
    dys = [exact_operand(M, N, seed=seed + 2 * i) for i in range(2 if acc else 1)]
    xs = [exact_operand(M, K, seed=seed + 2 * i + 1) for i in range(2 if acc else 1)]
    a0 = exact_operand(N, K, seed=seed + 9) * float(M) ** 0.5 if acc else None
    want = sum(dy.double().t() @ x.double() for dy, x in zip(dys, xs)) + (0 if a0 is None else a0.double())
    dd = [(dy.to(dev, dtype), x.to(dev, dtype)) for dy, x in zip(dys, xs)]

    def run():
        if not acc:
            return ops.weight_grad(*dd[0], fp32=fp32)
        a = a0.to(dev)
        for dy, x in dd:
            assert ops.weight_grad(dy, x, fp32=True, acc=a) is None
        return a
    got = _warm_then_fill(dev, run)
    if acc or fp32:
        assert got.dtype == torch.float32
    return got, want


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("entry", _entries("weight_grad"))
def test_weight_grad_entry(dev, dtype, entry):
    M, N, K, fp32, acc = entry
    got, want = _wgrad_case(dev, dtype, M, N, K, fp32, acc, _seed("wg", entry))
    _check("weight_grad", dtype, entry, "dW", got, want, N)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("M", [32, 128, 132, 2048])
def test_weight_grad_fp32_accumulate_token_counts(dev, dtype, M):
    """the adapter's dW over B * La token rows at batch 4 for La = 8, 32, 33 and 512 (M padded to 64 inside: a ragged pad tile
    and a reduction longer than one tile), two calls onto a prefilled fp32 accumulator"""
    got, want = _wgrad_case(dev, dtype, M, 384, 768, True, True, _seed("wgM", M))
    _check("weight_grad/M", dtype, (M, 384, 768), "dW", got, want, 384)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("entry", _entries("linear_dgrad"))
def test_linear_dgrad_entry(dev, dtype, entry):
    """dx = dy . W of a frozen Linear (autograd._Linear.backward: apad_gemm on the cached W^T)"""
    from ap_adapter_amd import autograd as AG
    M, N, K = entry
    s = _seed("lin", M, N, K)
    x, dy = exact_operand(M, K, seed=s), exact_operand(M, N, seed=s + 1)
    w = exact_operand(N, K, seed=s + 2, std=N ** -0.5)
    want = _cached(("lin", entry), lambda: dy.double() @ w.double())
    xd, wd, dyd = x.to(dev, dtype), w.to(dev, dtype), dy.to(dev, dtype)

    def run():
        xl = xd.clone().requires_grad_(True)
        AG.linear(xl, wd).backward(dyd)
        return xl.grad
    got = _warm_then_fill(dev, run)
    _check("linear_dgrad", dtype, entry, "dx", got, want, M)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("entry", _entries("conv_dgrad"))
def test_conv_dgrad_entry(dev, dtype, entry):
    """input gradient of the 3x3 convolution (stride 1; stride 2 through zero_stuff2; nearest upsample through upsample_nearest_bwd)"""
    from ap_adapter_amd import autograd as AG
    B, H, W, Cin, Cout, mode = entry
    stride, up = (2, None) if mode == "s2" else (1, None if mode == "s1" else tuple(mode))
    s = _seed("conv", entry)
    w = exact_operand(Cout, Cin, 3, 3, seed=s, std=(9 * Cout) ** -0.5)
    x = exact_operand(B, H * W, Cin, seed=s + 1)
    Hs, Ws = up if up is not None else (H, W)
    Ho, Wo = (Hs - 1) // stride + 1, (Ws - 1) // stride + 1
    dy = exact_operand(B, Ho * Wo, Cout, seed=s + 2)

    def make():
        xl = x.double().reshape(B, H, W, Cin).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        src = xl if up is None else F.interpolate(xl, size=up, mode="nearest")
        F.conv2d(src, w.double(), stride=stride, padding=1).backward(dy.double().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2))
        return xl.grad.permute(0, 2, 3, 1).contiguous()  # [B, H, W, Cin]
    want = _cached(("conv", entry), make)
    xd, wd, dyd = x.to(dev, dtype), w.to(dev, dtype), dy.to(dev, dtype)

    def run():
        xl = xd.clone().requires_grad_(True)
        out, ho, wo = AG.conv3x3(xl, wd, None, B, H, W, stride=stride, up=up)
        assert (ho, wo) == (Ho, Wo)
        out.backward(dyd)
        return xl.grad
    got = _warm_then_fill(dev, run)
    _check("conv_dgrad", dtype, entry, "dx", got.reshape(B, H, W, Cin), want, B * H)

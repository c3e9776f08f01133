"""-m gpu: the "high" fp32 matmul precision (APAD_F32_BF16X3: gemm_f32x3_kernel / attn_f32x3_kernel on split operands).

Parity is stated against fp64 torch on the fp32 operands, and bounded by the error of the EXACT bf16x3 product -- the three partial
products hi.hi + hi.lo + lo.hi of the test's own split, summed in fp64: the kernels may add fp32 accumulation on top of that, not more
than 4x.  The gain over 16-bit storage is asserted against the fp64 product of the bf16-rounded operands (a lower bound of what a
bf16-storage apad_gemm gives).  Every test leaves the precision at "highest"."""
import pytest
import torch
import torch.nn.functional as F

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture
def high():
    A.set_float32_matmul_precision("high")
    try:
        yield
    finally:
        A.set_float32_matmul_precision("highest")


def _count():
    return int(L.lib().apad_f32x3_launch_count())


def _split(x):
    hi = x.float().to(torch.bfloat16).double()
    lo = (x.float() - hi.float()).to(torch.bfloat16).double()
    return hi, lo


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _parity(run, bil, epi, a, w, launches):
    """run(): the op on the GPU in "high" -> fp32 result; bil(a, w) its bilinear part in fp64, epi(pre) the rest in fp64."""
    n0 = _count()
    out = run().double().cpu()
    torch.cuda.synchronize()
    assert _count() - n0 == launches
    a64, w64 = a.double(), w.double()
    (ah, al), (wh, wl) = _split(a), _split(w)
    ref = epi(bil(a64, w64))
    x3 = epi(bil(ah, wh + wl) + bil(al, wh))  # hi.hi + hi.lo + lo.hi (bil is linear in w)
    b16 = epi(bil(a.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()))
    err, err3, err16 = (float((t - ref).abs().max()) for t in (out, x3, b16))
    assert err <= 4 * err3, (err, err3)
    assert 30 * err <= err16, (err, err16)
    return out


def _linear_bil(a, w):
    return a @ w.t()


@pytest.mark.parametrize("M,N,K", [(1000, 640, 644), (64, 1280, 1284), (77, 36, 12), (130, 100, 20)])
@pytest.mark.parametrize("act", [None, "silu", "gelu", "tanh", "gelu_tanh"])
def test_linear_epilogues(dev, high, M, N, K, act):
    x, w, b = _rnd(M, K, seed=1), _rnd(N, K, seed=2, scale=K ** -0.5), _rnd(N, seed=3, scale=0.1)
    res = _rnd(M, N, seed=4)
    f = {None: lambda t: t, "silu": F.silu, "gelu": F.gelu, "tanh": torch.tanh, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh")}[act]
    run = lambda: ops.linear(x.to(dev), w.to(dev), b.to(dev), residual=res.to(dev), act=act)
    _parity(run, _linear_bil, lambda p: f(p + b.double()) + res.double(), x, w, 1)


@pytest.mark.parametrize("act", ["geglu", "geglu_tanh"])
def test_linear_geglu(dev, high, act):
    M, N, K = 200, 96, 324
    x, w, b = _rnd(M, K, seed=5), _rnd(2 * N, K, seed=6, scale=K ** -0.5), _rnd(2 * N, seed=7, scale=0.1)
    g = (lambda t: F.gelu(t, approximate="tanh")) if act == "geglu_tanh" else F.gelu
    run = lambda: ops.linear(x.to(dev), w.to(dev), b.to(dev), act=act)
    epi = lambda p: (p[:, :N] + b[:N].double()) * g(p[:, N:] + b[N:].double())
    _parity(run, _linear_bil, epi, x, w, 1)


def test_linear_rowgroup_bias(dev, high):
    M, N, K, rpg = 192, 128, 132, 64
    x, w = _rnd(M, K, seed=8), _rnd(N, K, seed=9, scale=K ** -0.5)
    rg = _rnd(5, N, seed=10)
    step = torch.tensor([1], dtype=torch.int32)
    run = lambda: ops.linear(x.to(dev), w.to(dev), act="silu", rowgroup_bias=rg.to(dev), rows_per_group=rpg, step_ptr=step.to(dev))
    rows = rg.double()[torch.arange(M) // rpg + 1]
    _parity(run, _linear_bil, lambda p: F.silu(p + rows), x, w, 1)


def _conv_bil(stride, up=None, asym=False):
    def bil(x, w):  # x [B, H, W, C] (channels last, as the kernel reads it), w [Cout, Cin, 3, 3]
        t = x.permute(0, 3, 1, 2)
        if up is not None:
            t = F.interpolate(t, size=up, mode="nearest")
        t = F.pad(t, (0, 1, 0, 1)) if asym else F.pad(t, (1, 1, 1, 1))
        return F.conv2d(t, w, stride=stride).permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    return bil


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up,asym", [
    (1, 125, 8, 640, 640, 1, None, False),   # the 1000-pixel level
    (2, 32, 2, 1280, 1280, 1, None, False),  # the 64-pixel level (two samples)
    (1, 50, 8, 20, 36, 2, None, False),      # down-sampler
    (2, 16, 2, 64, 44, 1, (32, 4), False),   # up-sampler (nearest x2)
    (1, 20, 10, 12, 8, 2, None, True),       # the VAE encoder's asymmetric down-sampler
])
def test_conv3x3(dev, high, B, H, W, Cin, Cout, stride, up, asym):
    x, w, b = _rnd(B, H, W, Cin, seed=11), _rnd(Cout, Cin, 3, 3, seed=12, scale=(9 * Cin) ** -0.5), _rnd(Cout, seed=13, scale=0.1)

    def run():
        o, Ho, Wo = ops.conv3x3(x.reshape(B, H * W, Cin).to(dev), ops.conv3x3_weight(w.to(dev)), b.to(dev), B, H, W, stride=stride, up=up,
                                asym_pad=asym)
        return o.reshape(-1, Cout)
    _parity(run, _conv_bil(stride, up, asym), lambda p: p + b.double(), x, w, 1)


@pytest.mark.parametrize("taps,dilation,transposed,pre,act", [(7, 1, 0, None, None), (3, 5, 0, 0.1, None), (3, 1, 0, None, "tanh"),
                                                                (16, 1, 8, 0.1, None)])
def test_conv1d(dev, high, taps, dilation, transposed, pre, act):
    B, T, Cin, Cout = 2, 37, 36, 20
    x = _rnd(B, T, Cin, seed=14)
    w = _rnd(Cout, taps, Cin, seed=15, scale=(taps * Cin) ** -0.5)
    b = _rnd(Cout, seed=16, scale=0.1)
    pad = (taps - transposed) // 2 if transposed else (taps * dilation - dilation) // 2
    xa = torch.where(x > 0, x, x * pre) if pre is not None else x  # the kernel splits the pre-activated value (same fp32 multiply)
    run = lambda: ops.conv1d(x.to(dev), w.reshape(Cout, -1).to(dev), b.to(dev), taps, dilation, transposed, pad, pre, act=act).reshape(-1, Cout)
    f = torch.tanh if act == "tanh" else (lambda t: t)
    if transposed:  # against conv_transpose1d, whose weight [Cin, Cout, taps] is the packed w re-ordered
        bil = lambda xx, ww: F.conv_transpose1d(xx.permute(0, 2, 1), ww.permute(2, 0, 1), stride=transposed, padding=pad).permute(0, 2, 1).reshape(-1, Cout)
    else:
        bil = lambda xx, ww: F.conv1d(xx.permute(0, 2, 1), ww.permute(0, 2, 1), dilation=dilation, padding=pad).permute(0, 2, 1).reshape(-1, Cout)
    _parity(run, bil, lambda p: f(p + b.double()), xa, w, 1)


def test_patch16(dev, high):
    B, H, W = 2, 64, 32
    mel, w, b = _rnd(B, H, W, seed=17), _rnd(768, 256, seed=18, scale=1 / 16), _rnd(768, seed=19, scale=0.1)
    run = lambda: ops.patch_embed(mel.to(dev), w.to(dev), b.to(dev), torch.float32).reshape(-1, 768)
    bil = lambda m, ww: F.conv2d(m[:, None], ww.reshape(768, 1, 16, 16), stride=16).permute(0, 2, 3, 1).reshape(-1, 768)
    _parity(run, bil, lambda p: p + b.double(), mel, w, 1)


def test_qkv_and_vt_outputs(dev, high):
    B, Lk, heads, d, K = 2, 45, 4, 16, 68
    Cc = heads * d
    x, w, b = _rnd(B * Lk, K, seed=20), _rnd(3 * Cc, K, seed=21, scale=K ** -0.5), _rnd(3 * Cc, seed=22, scale=0.1)
    Lpad = 64

    def run_qkv():
        q = torch.empty(B * Lk, Cc, device=dev)
        k = torch.empty(B * Lk, Cc, device=dev)
        vt = torch.zeros(B, heads, d, Lpad, device=dev)
        ops.linear_qkv(x.to(dev), w.to(dev), B, Lk, heads, q, k, vt, bias=b.to(dev))
        v = vt[..., :Lk].permute(0, 3, 1, 2).reshape(B * Lk, Cc)
        return torch.cat([q, k, v], 1)
    _parity(run_qkv, _linear_bil, lambda p: p + b.double(), x, w, 1)

    wv, bv = w[2 * Cc:].contiguous(), b[2 * Cc:].contiguous()

    def run_vt():
        vt = torch.zeros(B, heads, d, Lpad, device=dev)
        ops.linear_vt(x.to(dev), wv.to(dev), B, Lk, heads, vt, bias=bv.to(dev))
        return vt[..., :Lk].permute(0, 3, 1, 2).reshape(B * Lk, Cc)
    _parity(run_vt, _linear_bil, lambda p: p + bv.double(), x, wv, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def _vt(v, heads, Lpad):
    B, Lk, Cc = v.shape
    out = torch.zeros(B, heads, Cc // heads, Lpad)
    out[..., :Lk] = v.reshape(B, Lk, heads, Cc // heads).permute(0, 2, 3, 1)
    return out


def _attn_ref(q, k, v, heads, mm, split_p, bias=None, base2=False):
    """fp64 attention with the products formed by mm(a, b) = a @ b^T; split_p: P (un-normalised, relative to the row max, as the
    kernel holds it) goes through the fp32 split too.  Returns (out [B, N, C], lse base 2 [B, heads, N])."""
    B, N, Cc = q.shape
    d = Cc // heads
    qh = q.reshape(B, N, heads, d).transpose(1, 2)
    kh = k.reshape(B, -1, heads, d).transpose(1, 2)
    vh = v.reshape(B, -1, heads, d).transpose(1, 2)
    s = mm(qh, kh) * (1.0 if base2 else d ** -0.5 * 1.4426950408889634)  # base-2 exponents
    if bias is not None:
        s = s + bias.double()[:, None, None, :] * 1.4426950408889634
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2(s - mx)
    den = p.sum(-1, keepdim=True)
    o = (mm(p, vh.transpose(-1, -2)) if split_p else p @ vh) / den
    lse = (mx + torch.log2(den))[..., 0]
    return o.transpose(1, 2).reshape(B, N, Cc), lse


def _mm_exact(a, b):
    return a @ b.transpose(-1, -2)


def _mm_x3(a, b):
    (ah, al), (bh, bl) = _split(a), _split(b)
    return ah @ bh.transpose(-1, -2) + ah @ bl.transpose(-1, -2) + al @ bh.transpose(-1, -2)


def _mm_bf16(a, b):
    return a.float().to(torch.bfloat16).double() @ b.float().to(torch.bfloat16).double().transpose(-1, -2)


@pytest.mark.parametrize("D", [16, 32, 48, 64, 80, 96, 128])
@pytest.mark.parametrize("L2", [0, 1, 64, 65, 512])
def test_attention_parity(dev, high, D, L2):
    heads, B, N, L1 = 2, 2, 100, 8
    Cc = heads * D
    q, k1, v1 = _rnd(B, N, Cc, seed=30), _rnd(B, L1, Cc, seed=31), _rnd(B, L1, Cc, seed=32)
    k2, v2 = _rnd(B, max(L2, 1), Cc, seed=33), _rnd(B, max(L2, 1), Cc, seed=34)
    s2 = 0.55
    n0 = _count()
    kw = {}
    if L2:
        kw = dict(k2=k2.to(dev), vt2=_vt(v2, heads, (L2 + 31) // 32 * 32).to(dev), L2=L2, scale2=s2)
    out = ops.attention(q.to(dev), k1.to(dev), _vt(v1, heads, 32).to(dev), L1, heads, **kw).double().cpu()
    assert _count() - n0 == 1

    def ref(mm, split_p):
        o, _ = _attn_ref(q.double(), k1.double(), v1.double(), heads, mm, split_p)
        if L2:
            o = o + s2 * _attn_ref(q.double(), k2.double(), v2.double(), heads, mm, split_p)[0]
        return o
    exact, x3, b16 = ref(_mm_exact, False), ref(_mm_x3, True), ref(_mm_bf16, True)
    err, err3, err16 = (float((t - exact).abs().max()) for t in (out, x3, b16))
    assert err <= 4 * err3, (err, err3)
    assert 30 * err <= err16, (err, err16)


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_key_bias_lse_prescaled(dev, high, D, prescaled):
    heads, B, N, Lk = 2, 3, 70, 77
    Cc = heads * D
    q, k, v = _rnd(B, N, Cc, seed=40), _rnd(B, Lk, Cc, seed=41), _rnd(B, Lk, Cc, seed=42)
    if prescaled:
        q = q * (D ** -0.5 * 1.4426950408889634)
    bias = torch.zeros(B, Lk)
    bias[1, -10:] = -1e4  # a padding mask as an additive bias
    bias[2] = _rnd(Lk, seed=43)
    n0 = _count()
    if prescaled:
        out = ops.attention(q.to(dev), k.to(dev), _vt(v, heads, 96).to(dev), Lk, heads, key_bias=bias.to(dev), q_prescaled=True)
        lse = None
    else:
        out, lse = ops.attention_lse(q.to(dev), k.to(dev), _vt(v, heads, 96).to(dev), Lk, heads, key_bias=bias.to(dev))
    out = out.double().cpu()
    assert _count() - n0 == 1
    refs = {name: _attn_ref(q.double(), k.double(), v.double(), heads, mm, sp, bias, base2=prescaled)
            for name, mm, sp in (("exact", _mm_exact, False), ("x3", _mm_x3, True), ("b16", _mm_bf16, True))}
    err, err3, err16 = (float((t - refs["exact"][0]).abs().max()) for t in (out, refs["x3"][0], refs["b16"][0]))
    assert err <= 4 * err3, (err, err3)
    assert 30 * err <= err16, (err, err16)
    if lse is not None:
        lse = lse.double().cpu()[..., :N]
        e, e3 = (float((t - refs["exact"][1]).abs().max()) for t in (lse, refs["x3"][1]))
        assert e <= 4 * e3 + 1e-6, (e, e3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the UNet / pipeline in "high"
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("La,scale,frames", [(32, 0.55, 250), (512, 1.0, 64)])
def test_full_geometry_noise_pred_high_within_north_star(dev, high, La, scale, frames):
    """the north-star bar (<= 1e-3 max-abs on noise_pred vs the oracle chain) in "high", the cases of the fp32 test"""
    from test_gpu_unet import _full_geometry_case
    n0 = _count()
    out, oracle = _full_geometry_case(dev, torch.float32, La, scale, frames=frames)
    launches = _count() - n0
    assert launches > 500, launches  # every projection, convolution and attention of the forward ran on the split kernels
    ref = oracle()
    err = float((out - ref).abs().max())
    print(f"\n[full-geometry noise_pred, fp32 high, La={La}] max-abs err={err:.3e}, {launches} bf16x3 launches")
    assert err <= 1e-3


def _small_f32(dev):
    from test_gpu_unet import _small_unet
    u, cfg, sd, procs = _small_unet(dev, torch.float32)
    u.requires_grad_(False)
    return u


def _small_inputs(dev, B, seed=2):
    from test_gpu_unet import _cond
    lat = torch.randn(B, 8, 26, 16, generator=torch.Generator().manual_seed(seed))
    ehs, ehs1, m1 = _cond(2 * B, 32, torch.float32, seed=seed)
    return lat.to(dev), ehs.to(dev), ehs1.to(dev), m1.to(dev)


def test_pipeline_graph_equals_eager_in_high(dev, high):
    u = _small_f32(dev)
    pipe = A.AudioLDM2Pipeline(u)
    inp = _small_inputs(dev, 2)
    a = pipe.denoise(*inp, 3, 7.5, use_graph=True)
    n0 = _count()
    b = pipe.denoise(*inp, 3, 7.5, use_graph=False)
    assert _count() > n0  # the eager run went through the split kernels
    assert torch.equal(a, b)


def test_clip_is_independent_of_its_batch_in_high(dev, high):
    u = _small_f32(dev)
    pipe = A.AudioLDM2Pipeline(u)
    lat, ehs, ehs1, m1 = _small_inputs(dev, 4, seed=5)
    four = pipe.denoise(lat, ehs, ehs1, m1, 2, 7.5, use_graph=False)
    i = 2
    cond = lambda t: torch.stack([t[i], t[4 + i]])  # CFG: unconditional half first, then conditional
    one = pipe.denoise(lat[i:i + 1], cond(ehs), cond(ehs1), cond(m1), 2, 7.5, use_graph=False)
    assert torch.equal(one[0], four[i])


def test_highest_is_untouched_by_a_high_excursion(dev):
    u = _small_f32(dev)
    x = torch.randn(2, 8, 26, 16, generator=torch.Generator().manual_seed(7)).to(dev)
    _, ehs, ehs1, m1 = _small_inputs(dev, 1)
    t = torch.tensor(301)
    fwd = lambda: u(x, t, encoder_hidden_states=ehs, encoder_hidden_states_1=ehs1, encoder_attention_mask_1=m1, return_dict=False)[0]
    with torch.no_grad():
        n0 = _count()
        before = fwd().clone()
        assert _count() == n0  # "highest" never launches a split kernel
        A.set_float32_matmul_precision("high")
        try:
            high_out = fwd().clone()
            assert _count() > n0
        finally:
            A.set_float32_matmul_precision("highest")
        n1 = _count()
        after = fwd()
        assert _count() == n1
    assert torch.equal(before, after)
    assert not torch.equal(before, high_out)
    assert float((before - high_out).abs().max()) < 1e-3


def test_graph_is_recaptured_after_a_precision_switch(dev):
    u = _small_f32(dev)
    pipe = A.AudioLDM2Pipeline(u)
    inp = _small_inputs(dev, 2)
    try:
        a = pipe.denoise(*inp, 2, 7.5)
        assert pipe.graph_captures == 1
        A.set_float32_matmul_precision("high")
        b = pipe.denoise(*inp, 2, 7.5)
        assert pipe.graph_captures == 2  # never the "highest" graph replayed
        A.set_float32_matmul_precision("highest")
        c = pipe.denoise(*inp, 2, 7.5)
        assert pipe.graph_captures == 2 and pipe.graph_hits == 1  # the first graph, replayed
    finally:
        A.set_float32_matmul_precision("highest")
    assert torch.equal(a, c)
    assert not torch.equal(a, b)


def test_split_weight_follows_a_parameter_update(dev, high):
    M, N, K = 64, 96, 132
    lin = torch.nn.Linear(K, N).to(dev)
    x = _rnd(M, K, seed=50).to(dev)
    with torch.no_grad():
        y0 = ops.linear(x, lin.weight, lin.bias).clone()
        s0 = ops.f32_split_weight(lin.weight, N, K, K)
        assert ops.f32_split_weight(lin.weight, N, K, K) is s0  # cached
        lin.weight.mul_(-0.5)  # an in-place update (what an optimizer step does)
        y1 = ops.linear(x, lin.weight, lin.bias)
        s1 = ops.f32_split_weight(lin.weight, N, K, K)
    assert s1 is not s0
    w = lin.weight.detach().cpu().double()
    ref = x.cpu().double() @ w.t() + lin.bias.detach().cpu().double()
    assert float((y1.cpu().double() - ref).abs().max()) < 1e-4
    assert float((y1 - y0).abs().max()) > 0.1
    hi, lo = _split(lin.weight.detach().cpu())
    assert torch.equal(s1[0].cpu().double(), hi) and torch.equal(s1[1].cpu().double(), lo)


def test_captured_training_step_follows_the_optimizer_in_high(dev, high):
    """the trainable adapter weights change between replays (AdamW writes them through raw pointers): the captured micro-step must split
    them inside the graph, so a replay after an optimizer step computes what an eager micro-step on the updated weights computes"""
    from test_gpu_train import _small_unet as _train_unet, _batch
    from oracle import train as OT
    u, cfg, sd, procs = _train_unet(dev, torch.float32)
    tr = A.AdapterTrainer(u, lr=1e-2)
    lat, noise, t, ehs, ehs1, m1 = _batch(2, 8, torch.float32)
    args = (OT.add_noise(lat, noise, t).to(dev), t.to(dev), ehs.to(dev), ehs1.to(dev), m1.to(dev), noise.to(dev))
    replay = tr.capture_micro_step(2, 26, 16, ehs.shape[1], ehs1.shape[1])
    loss0 = float(replay(*args))
    tr.optimizer_step()
    loss_g = float(replay(*args))
    grad_g = tr.grad.clone()
    tr.grad.zero_()
    tr._micro = 0
    n0 = _count()
    loss_e = float(tr.micro_step(*args))
    assert _count() > n0  # the forward ran on the split kernels
    assert loss_g != loss0  # the step moved the weights the replay read
    assert loss_g == loss_e and torch.equal(tr.grad, grad_g)


def test_hoisted_kv_follow_the_precision(dev):
    """with the K/V hoist on, a precision switch re-projects the hoisted K/V: "highest" after a "high" excursion is bit-equal to before"""
    u = _small_f32(dev)
    x = torch.randn(2, 8, 26, 16, generator=torch.Generator().manual_seed(8)).to(dev)
    _, ehs, ehs1, m1 = _small_inputs(dev, 1)
    t = torch.tensor(401)
    fwd = lambda: u(x, t, encoder_hidden_states=ehs, encoder_hidden_states_1=ehs1, encoder_attention_mask_1=m1, return_dict=False)[0].clone()
    with torch.no_grad():
        plain_highest = fwd()
        A.set_float32_matmul_precision("high")
        try:
            plain_high = fwd()
        finally:
            A.set_float32_matmul_precision("highest")
        u.set_kv_cache(True)
        try:
            before = fwd()
            A.set_float32_matmul_precision("high")
            try:
                hoisted_high = fwd()
            finally:
                A.set_float32_matmul_precision("highest")
            after = fwd()
        finally:
            u.set_kv_cache(False)
    assert torch.equal(before, plain_highest) and torch.equal(after, plain_highest)
    assert torch.equal(hoisted_high, plain_high)


def test_activation_operand_is_split_as_it_is_now(dev, high):
    """a buffer used as the second GEMM operand (the VAE / T5 attention) and rewritten by a kernel -- no version bump -- is split afresh"""
    M, N, K = 40, 48, 36
    a = _rnd(M, K, seed=60).to(dev)
    eye = torch.eye(K, device=dev)
    buf = torch.empty(N, K, device=dev)
    with torch.no_grad():
        ops.linear(_rnd(N, K, seed=61).to(dev), eye, out=buf)  # written by the library: buf._version does not move
        y1 = ops.gemm(a, buf, M=M, N=N, K=K, lda=K, out=torch.empty(M, N, device=dev), ldo=N).clone()
        v = buf._version
        ops.linear(_rnd(N, K, seed=62).to(dev), eye, out=buf)
        assert buf._version == v
        y2 = ops.gemm(a, buf, M=M, N=N, K=K, lda=K, out=torch.empty(M, N, device=dev), ldo=N)
    ref = a.double() @ buf.double().t()
    assert float((y2.double() - ref).abs().max()) < 1e-3  # (the split product: ~2^-16 of sum |a||w| over K = 36)
    assert float((y2 - y1).abs().max()) > 0.1

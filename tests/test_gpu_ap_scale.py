"""-m gpu: ap_scale from a device table -- the four apad_*_tab entry points against their scalar twins bit for bit (row, column, modulo, a
counter past the table, tiles that span two samples, rejected arguments), the UNet with a binding on every decoupled processor, and the
pipeline's ``ap_scale=`` keyword: schedules, sweeps on one captured graph, per-clip values, editing, inversion and three-branch guidance.

Nothing here has a tolerance except the inversion round trip (the bar of tests/test_gpu_invert.py): a table launch reads its value once per
workgroup and feeds it to the expression the descriptor's float feeds, so every comparison with the scalar path is ``torch.equal``."""
import ctypes as C

import pytest
import torch

from util import nan_fill_free, rel_err

from test_gpu_unet import _cond, _small_unet

pytestmark = pytest.mark.gpu
NAN = float("nan")
VALUES = (0.25, 0.55, -1.5)  # three different weights, one negative: the reference constrains nothing


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    nan_fill_free(dev)


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: one launcher per entry point and route
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = {  # name: (op, C, dtype, fp32 precision or None)
    "attention-bf16": ("attention", 256, torch.bfloat16, None), "attention-f16": ("attention", 256, torch.float16, None),
    "attention-f32": ("attention", 256, torch.float32, "highest"), "attention-f32-high": ("attention", 256, torch.float32, "high"),
    "fused-bf16": ("fused", 256, torch.bfloat16, None), "fused-f16": ("fused", 256, torch.float16, None),
    "rows-bf16": ("rows", 384, torch.bfloat16, None), "rows-f16": ("rows", 384, torch.float16, None),
    "hs-bf16": ("hs", 640, torch.bfloat16, None), "hs-f16": ("hs", 640, torch.float16, None),
}
ENTRY = {"attention": "apad_attention", "fused": "apad_fused_cross_attention", "rows": "apad_cross_attention_rows", "hs": "apad_hs_attention"}


def _launcher(dev, route, B, N, La, Lt=8, seed=900):
    """random operands of one route on the device -> launch(scale2) -> a NaN-prefilled output the launch wrote (no key bias: the long
    forms' envelope); La = 0 is the single-segment call"""
    from ap_adapter_amd import ops
    op, C_, dtype, _ = ROUTES[route]
    H = 8
    d = C_ // H
    D = lambda t: t.to(dev, dtype).contiguous()
    x = D(R(B, N, C_, seed=seed))
    g, be = D(1 + 0.1 * R(C_, seed=seed + 1)), D(0.1 * R(C_, seed=seed + 2))
    wq, wo, bo = D(R(C_, C_, seed=seed + 3, std=0.05)), D(R(C_, C_, seed=seed + 4, std=0.05)), D(R(C_, seed=seed + 5, std=0.3))

    def kv(L, s):
        if not L:
            return None, None
        vt = torch.zeros(B, H, d, ops.round_up(L, 32), device=dev, dtype=dtype)
        vt[..., :L] = D(R(B, H, d, L, seed=s))
        return D(R(B, L, C_, seed=s + 1, std=0.5)), vt

    (k1, v1t), (k2, v2t) = kv(Lt, seed + 6), kv(La, seed + 8)
    ln = (g, be, 1e-5)
    out = torch.empty_like(x)
    if op == "attention":
        def launch(scale2):
            return ops.attention(x, k1, v1t, Lt, H, k2=k2, vt2=v2t, L2=La, scale2=scale2, out=out.fill_(NAN))
    elif op == "fused":
        (wq_p, q_fold), wo_p = ops.xattn_pack_weight(wq, ln), ops.xattn_pack_weight(wo)
        pk1, pk2 = ops.xattn_pack_kv(k1, v1t, Lt), (ops.xattn_pack_kv(k2, v2t, La) if La else None)

        def launch(scale2):
            return ops.fused_cross_attention(x, wq_p, wo_p, bo, pk1, Lt, H, ln=ln, kv2_packed=pk2, L2=La, scale2=scale2, q_fold=q_fold,
                                             out=out.fill_(NAN))
    elif op == "rows":
        wq_p, wo_p = ops.xrows_pack_weight(wq), ops.xrows_pack_weight(wo)

        def launch(scale2):
            return ops.cross_attention_rows(x, wq_p, wo_p, bo, k1, v1t, H, ln=ln, k2=k2, vt2=v2t, scale2=scale2, out=out.fill_(NAN))
    else:
        wq_p, qb = ops.hs_pack_rows(wq, ln=ln)

        def launch(scale2):
            return ops.hs_attention(x, wq_p, qb, self_attention=False, ln_eps=1e-5, k1=k1, vt1=v1t, k2=k2, vt2=v2t, scale2=scale2,
                                    out=out.fill_(NAN))
    return launch


class _precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from ap_adapter_amd import ops
        self.was = ops.get_float32_matmul_precision()
        if self.mode is not None:
            ops.set_float32_matmul_precision(self.mode)

    def __exit__(self, *exc):
        from ap_adapter_amd import ops
        ops.set_float32_matmul_precision(self.was)


def _cases():
    out = []
    for route, (op, _, _, _) in ROUTES.items():
        if op == "attention":  # L2 <= 64: the short-segment kernel; above: the tiled one (fp32: one kernel, both lengths)
            shapes = [(100, 32), (100, 128)]
        elif op == "fused":  # three panels per sample: a four-panel tile spans two samples (N = 96), or not (128); resident (32), big (128) and chunked (192) segment 2
            shapes = [(96, 32), (128, 32), (96, 128), (128, 128), (96, 192), (128, 192)]
        elif op == "rows":  # a ragged last tile (40) and whole 64-token tiles (128); resident and chunked running-max forms
            shapes = [(40, 32), (128, 32), (40, 128), (128, 128)]
        else:  # the 64-token level: ragged and full samples
            shapes = [(40, 32), (64, 32), (40, 128), (64, 128)]
        out += [(route, n, la) for n, la in shapes]
    return out


@pytest.mark.parametrize("route,N,La", _cases())
def test_table_launch_equals_the_scalar_launch_bit_for_bit(dev, route, N, La):
    """B = 3 samples, a table of 4 rows whose read row holds three DIFFERENT values and whose other rows are NaN: the output rows of sample b
    are the bits of the scalar launch with value_b (the row and the column were read, and the arithmetic is the existing one); then the
    one-column broadcast, a counter past the table (reads the last row), no counter (row 0), and B = 6 samples on 3 columns (rows b and
    b + 3 share a column)."""
    from ap_adapter_amd import ops
    with _precision(ROUTES[route][3]):
        launch = _launcher(dev, route, 3, N, La)
        scalar = [launch(v).clone() for v in VALUES]
        assert all(bool(torch.isfinite(s).all()) for s in scalar)
        for b in range(3):  # the weight matters, on every sample
            assert not torch.equal(scalar[0][b], scalar[1][b]) and not torch.equal(scalar[1][b], scalar[2][b])
        step = torch.full((1,), 2, dtype=torch.int32, device=dev)
        table = torch.full((4, 3), NAN, device=dev)
        table[2] = torch.tensor(VALUES)
        out = launch(ops.Scale2Binding(table, step, 3)).clone()
        for b in range(3):
            assert torch.equal(out[b], scalar[b][b]), (route, b)
        # a plain tuple is a binding too; cols = 1: every sample reads column 0
        one = torch.full((4, 1), NAN, device=dev)
        one[2] = VALUES[1]
        assert torch.equal(launch((one, step, 1)), scalar[1])
        wide = torch.full((4, 3), NAN, device=dev)  # ld = 3 > cols = 1
        wide[2, 0] = VALUES[2]
        assert torch.equal(launch((wide, step, 1)), scalar[2])
        # a counter past the table reads the last row, never past it; no counter: row 0
        last = torch.full((4, 3), NAN, device=dev)
        last[3] = torch.tensor(VALUES)
        step.fill_(1000)
        assert torch.equal(launch((last, step, 3)), out)
        first = torch.full((4, 3), NAN, device=dev)
        first[0] = torch.tensor(VALUES)
        assert torch.equal(launch((first, None, 3)), out)
        # cols = 3 with B = 6: the modulo maps the branches of a clip onto one column
        launch6 = _launcher(dev, route, 6, N, La)
        scalar6 = [launch6(v).clone() for v in VALUES]
        step.fill_(2)
        out6 = launch6((table, step, 3))
        for b in range(6):
            assert torch.equal(out6[b], scalar6[b % 3][b]), (route, b)


def test_rows_entry_point_keeps_its_envelope(dev):
    """apad_cross_attention_rows serves C = 384 only (the 640-wide level is apad_hs_attention's, covered above): the _tab entry refuses what
    its twin refuses"""
    from ap_adapter_amd import ops
    x = torch.zeros(2, 40, 640, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="outside the kernel envelope"):
        ops.cross_attention_rows(x, x, x, None, torch.zeros(2, 8, 640, device=dev, dtype=torch.bfloat16), None, 8,
                                 scale2=(torch.zeros(1, 1, device=dev), None, 1))


@pytest.mark.parametrize("route", ["attention-bf16", "attention-f32", "fused-bf16", "rows-bf16", "hs-bf16"])
def test_rejected_tables_are_errors_and_launch_nothing(dev, route, monkeypatch):
    """every rejected argument of the C ABI: refused by the wrapper (RuntimeError) and by the raw entry point (a negative code and a text
    naming it), the NaN-prefilled output untouched afterwards"""
    from ap_adapter_amd import _lib as L, ops
    name = ENTRY[ROUTES[route][0]] + "_tab"
    lib = L.lib()
    real = getattr(lib, name)
    seen = []
    monkeypatch.setattr(lib, name, lambda d, t, s: (seen.append((d._obj, t._obj)), real(d, t, s))[1])
    with _precision(ROUTES[route][3]):
        launch, single = _launcher(dev, route, 3, 40, 32), _launcher(dev, route, 3, 40, 0)
        good = torch.full((4, 3), 0.5, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        done = launch((good, step, 3))
        assert bool(torch.isfinite(done).all()) and len(seen) == 1
        desc, tab = seen[0]
        untouched = lambda: bool(torch.isnan(done).all())
        bad = {"a null table": (None, step, 3), "rows <= 0": (torch.empty(0, 3, device=dev), step, 3), "cols <= 0": (good, step, 0),
               "negative cols": (good, step, -2), "ld < cols": (good[:, :2].contiguous(), step, 3)}
        for what, binding in bad.items():
            with pytest.raises(RuntimeError, match=name):
                launch(binding)
            assert untouched(), what
        with pytest.raises(RuntimeError, match=name + ".*second segment"):  # a table given to a single-segment call
            single((good, step, 3))
        assert untouched()
        # what the wrapper checks itself: device, dtype, contiguity, shape
        for what, binding in {"host table": (good.cpu(), step, 3), "fp64 table": (good.double(), step, 3), "strided table": (good.t(), step, 3),
                              "1-D table": (good[0], step, 3), "int64 counter": (good, step.long(), 3),
                              "two counters": (good, torch.zeros(2, dtype=torch.int32, device=dev), 3), "host counter": (good, step.cpu(), 3)}.items():
            n = len(seen)
            with pytest.raises(RuntimeError):
                launch(binding)
            assert len(seen) == n and untouched(), what
        # the raw entry point, on the descriptor of the launch that worked
        monkeypatch.undo()
        done.fill_(NAN)

        def raw(**change):
            t = L.Scale2Tab()
            for f, _ in L.Scale2Tab._fields_:
                setattr(t, f, change.get(f, getattr(tab, f)))
            rc = real(C.byref(desc), C.byref(t), None)
            text = lib.apad_last_error().decode()
            torch.cuda.synchronize()
            return rc, text

        for change in (dict(table=None), dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-1), dict(ld=2), dict(table=tab.table + 2)):
            rc, text = raw(**change)
            assert rc < 0 and text.startswith(name + ":") and untouched(), (change, rc, text)
        l2 = desc.L2
        desc.L2 = 0
        rc, text = raw()
        desc.L2 = l2
        assert rc < 0 and text.startswith(name + ":") and untouched()
        assert real(C.byref(desc), None, None) < 0 and untouched()
        rc, text = raw()  # and unchanged it still launches
        assert rc == 0 and bool(torch.isfinite(done).all()), text


# ---------------------------------------------------------------------------------------------------------------------
# UNet level (small synthetic UNet, bf16)
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(dev, dtype, B=2, H=26, W=16, seed=2):
    lat = torch.randn(B, 8, H, W, generator=torch.Generator().manual_seed(seed))
    ehs, ehs1, m1 = _cond(2 * B, 32, dtype, seed=seed)
    return lat.to(dev), ehs.to(dev), ehs1.to(dev), m1.to(dev)


def _ip(u):
    return [p for p in set(u.attn_processors.values()) if hasattr(p, "to_k_ip")]


class _scales:
    """every decoupled processor's ``scale`` set to one value, put back afterwards"""

    def __init__(self, u, value):
        self.procs, self.value = _ip(u), value

    def __enter__(self):
        self.was = [p.scale for p in self.procs]
        for p in self.procs:
            p.scale = self.value

    def __exit__(self, *exc):
        for p, s in zip(self.procs, self.was):
            p.scale = s


def _forward_with(u, dev, dtype, x, cond, repeat, table=None, row=1):
    from test_gpu_dual_guidance import _forward
    if table is None:
        return _forward(u, dev, dtype, x, cond, repeat)
    u.set_ap_scale_table(table, torch.full((1,), row, dtype=torch.int32, device=dev))
    try:
        return _forward(u, dev, dtype, x, cond, repeat)
    finally:
        u.clear_ap_scale_table()


def _table(dev, row_values, rows=3, row=1):
    t = torch.full((rows, len(row_values)), NAN, device=dev)
    t[row] = torch.tensor(row_values)
    return t


@pytest.mark.parametrize("chain", [False, True])
def test_unet_binding_with_the_processors_own_scale_changes_nothing(dev, monkeypatch, chain):
    """a binding holding 0.5, the processors' own ``scale``: the forward is the forward without a binding, bit for bit -- on the fused routes,
    and on the chain with the fused routes switched off (apad_attention_tab)"""
    from ap_adapter_amd import _lib as L, ops
    from ap_adapter_amd import processors as P
    dtype = torch.bfloat16
    u = _small_unet(dev, dtype)[0]
    u.requires_grad_(False)
    if chain:
        monkeypatch.setattr(P, "USE_FUSED_XATTN", False)
        for name in ("HS_ATTN", "SATTN_FUSED", "MLP_PACKED"):
            monkeypatch.setattr(ops, name, False)
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    x = lat.float().permute(0, 2, 3, 1).reshape(2, 26 * 16, 8).to(dtype).contiguous()
    lib, calls = L.lib(), {}
    for op in ENTRY.values():
        for name in (op, op + "_tab"):
            monkeypatch.setattr(lib, name, (lambda real, n: lambda *a: (calls.__setitem__(n, calls.get(n, 0) + 1), real(*a))[1])(getattr(lib, name), name))
    plain = _forward_with(u, dev, dtype, x, (ehs, ehs1, m1), 2)
    assert not any(n.endswith("_tab") for n in calls)
    before = dict(calls)
    calls.clear()
    bound = _forward_with(u, dev, dtype, x, (ehs, ehs1, m1), 2, _table(dev, [0.5]))
    assert torch.equal(bound, plain) and bool(torch.isfinite(plain).all())
    n_tab = sum(v for n, v in calls.items() if n.endswith("_tab"))
    assert n_tab >= len(A_ip_sites(u)) > 0, calls          # every decoupled site went through a _tab entry point ...
    assert sum(calls.values()) == sum(before.values())     # ... and nothing else moved
    if chain:
        assert set(n for n in calls if n.endswith("_tab")) == {"apad_attention_tab"}
    assert all(p.scale == 0.5 and p.scale_table is None for p in _ip(u))
    with _scales(u, 0.25):  # while a table is set, ``scale`` is not read
        assert torch.equal(_forward_with(u, dev, dtype, x, (ehs, ehs1, m1), 2, _table(dev, [0.5])), plain)
        assert not torch.equal(_forward_with(u, dev, dtype, x, (ehs, ehs1, m1), 2), plain)


def A_ip_sites(u):
    import ap_adapter_amd as A
    return A.ip_layer_names(u)


@pytest.mark.parametrize("repeat", [2, 3])
def test_unet_per_clip_columns_equal_the_scalar_forwards(dev, repeat):
    """column values (a, b) at B = 2: the rows of clip 0 -- in every guidance branch -- are the forward with every proc.scale = a, those of
    clip 1 the one with b, bit for bit; at batch_repeat = 2 and 3"""
    dtype = torch.bfloat16
    u = _small_unet(dev, dtype)[0]
    u.requires_grad_(False)
    B, (a, b) = 2, (0.125, 1.75)
    if repeat == 2:
        lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    else:
        from test_gpu_dual_guidance import _inputs3
        lat, ehs, ehs1, m1 = _inputs3(dev, dtype)
    x = lat.float().permute(0, 2, 3, 1).reshape(B, 26 * 16, 8).to(dtype).contiguous()
    cond = (ehs, ehs1, m1)
    both = _forward_with(u, dev, dtype, x, cond, repeat, _table(dev, [a, b]))
    assert both.shape[0] == repeat * B and bool(torch.isfinite(both).all())
    with _scales(u, a):
        fa = _forward_with(u, dev, dtype, x, cond, repeat)
    with _scales(u, b):
        fb = _forward_with(u, dev, dtype, x, cond, repeat)
    differ = 0
    for r in range(repeat * B):
        want, other = (fa, fb) if r % B == 0 else (fb, fa)
        assert torch.equal(both[r], want[r]), r
        differ += not torch.equal(both[r], other[r])
    assert differ >= B  # (the branch without audio tokens' content still has the second segment: the weight matters in the audio branches at least)


def test_full_geometry_binding_on_the_fused_routes(dev, monkeypatch):
    """AudioLDM2-large geometry on a 2.56 s clip, bf16, where the decoupled sites take the one-launch routes (apad_fused_cross_attention at
    C = 256, apad_cross_attention_rows at 384, apad_hs_attention at 640): a binding holding the processors' own scale changes no bit and
    every site goes through a _tab entry point; two columns on the two samples equal the two scalar forwards row by row"""
    import ap_adapter_amd as A
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd.synthetic import synthetic_inputs
    from util import full_unet
    dtype, frames = torch.bfloat16, 64
    u = full_unet(0.55).to(dtype)
    u.requires_grad_(False)
    inp = synthetic_inputs(1, 32)
    ehs = A.AudioLDM2Pipeline(u).assemble_condition(inp["generated_prompt_embeds"], inp["audio_tokens"], inp["uncond_audio_tokens"], dtype)
    ehs1 = inp["prompt_embeds"].to(dtype)
    x = torch.cat([inp["latents"][:, :, :frames]] * 2).to(dtype).contiguous()
    u = u.to(dev)
    args = (x.to(dev), torch.tensor(501))
    kw = dict(encoder_hidden_states=ehs.to(dev), encoder_hidden_states_1=ehs1.to(dev), encoder_attention_mask_1=inp["attention_mask"].to(dev),
              return_dict=False)
    lib, calls = L.lib(), {}
    for op in ENTRY.values():
        name = op + "_tab"
        monkeypatch.setattr(lib, name, (lambda real, n: lambda *a: (calls.__setitem__(n, calls.get(n, 0) + 1), real(*a))[1])(getattr(lib, name), name))

    def run(table=None):
        with torch.no_grad():
            if table is None:
                return u(*args, **kw)[0].clone()
            u.set_ap_scale_table(table, torch.ones(1, dtype=torch.int32, device=dev))
            try:
                return u(*args, **kw)[0].clone()
            finally:
                u.clear_ap_scale_table()

    plain = run()
    assert not calls and bool(torch.isfinite(plain).all())
    assert torch.equal(run(_table(dev, [0.55])), plain)
    print(f"\n[full geometry, bf16, frames={frames}] _tab launches per forward: {calls}")
    assert sum(calls.values()) == len(_ip(u)) == 32
    assert calls.get("apad_fused_cross_attention_tab", 0) > 0 and calls.get("apad_cross_attention_rows_tab", 0) > 0
    a, b = 0.2, 0.9
    both = run(_table(dev, [a, b]))
    with _scales(u, a):
        fa = run()
    with _scales(u, b):
        fb = run()
    assert torch.equal(both[0], fa[0]) and torch.equal(both[1], fb[1])
    assert not torch.equal(both[0], fb[0]) and not torch.equal(both[1], fa[1])


# ---------------------------------------------------------------------------------------------------------------------
# pipeline level
# ---------------------------------------------------------------------------------------------------------------------
STEPS, GS = 3, 7.5


def _pipe(dev, dtype, sampler="ddim"):
    import ap_adapter_amd as A
    u = _small_unet(dev, dtype)[0]
    u.requires_grad_(False)
    return A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler() if sampler == "dpm" else A.DDIMScheduler())


def _hand_loop(pipe, dev, dtype, lat, ehs, ehs1, m1, scales, H=26, W=16):
    """the two-branch loop written out on the SCALAR path: every processor's ``scale`` set before each step's forward"""
    from ap_adapter_amd import ops
    u, sched = pipe.unet, pipe.scheduler
    B = lat.shape[0]
    sched.set_timesteps(len(scales))
    plan = sched.sampler_plan(0.0)
    coef = plan.table.to(dev)
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    x = lat.float().permute(0, 2, 3, 1).reshape(B, H * W, 8).contiguous()
    unet_in = x.to(dtype)
    hist = torch.zeros_like(x) if plan.needs_history else None
    with torch.no_grad():
        u.set_kv_cache(True)
        u.precompute_time_tables(sched.timesteps.to(dev), step_ptr)
        try:
            for s in scales:
                with _scales(u, s):
                    eps2 = u.forward_nhwc(unet_in, H, W, None, ehs.to(dtype), ehs1.to(dtype), None, m1, batch_repeat=2)
                if plan.legacy:
                    ops.cfg_ddim_step(eps2, x, unet_in, coef, step_ptr, GS)
                else:
                    ops.cfg_sampler_step(eps2, x, unet_in, coef, step_ptr, GS, None, hist, None)
                ops.step_advance(step_ptr)
        finally:
            u.clear_time_tables()
            u.set_kv_cache(False)
    return x.reshape(B, H, W, 8).permute(0, 3, 1, 2).contiguous()


def _floats(key, top=True):
    """every float in a graph key outside the scheduler's own share (element 13: its betas and eta)"""
    out = []
    for k in (key[:13] + key[14:] if top else key):
        if isinstance(k, (tuple, list)):
            out += _floats(tuple(k), False)
        elif isinstance(k, float):
            out.append(k)
    return out


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_schedule_captured_equals_eager_equals_the_hand_loop(dev, sampler):
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype, sampler)
    inp = _inputs(dev, dtype)
    sched = [1.0, 0.5, 0.25]
    captured = pipe.denoise(*inp, STEPS, GS, ap_scale=sched)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0)
    assert torch.equal(pipe.last_ap_scale, torch.tensor(sched).reshape(3, 1)) and pipe.last_ap_scale.device.type == "cpu"
    eager = pipe.denoise(*inp, STEPS, GS, ap_scale=sched, use_graph=False)
    hand = _hand_loop(pipe, dev, dtype, *inp, sched)
    assert torch.equal(captured, eager) and torch.equal(captured, hand) and bool(torch.isfinite(hand).all())
    assert not torch.equal(hand, _hand_loop(pipe, dev, dtype, *inp, [1.0, 1.0, 1.0]))  # the later steps' values are read
    assert all(p.scale == 0.5 and p.scale_table is None for p in _ip(pipe.unet))  # neither read nor changed, and the binding is gone


def test_sweep_and_schedule_replay_one_captured_graph(dev):
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    inp = _inputs(dev, dtype)
    runs = [0.25, 0.5, 1.0, [1.0, 0.5, 0.0]]
    outs = [pipe.denoise(*inp, STEPS, GS, ap_scale=v) for v in runs]
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 3) and len(pipe._graphs) == 1
    fresh = A.AudioLDM2Pipeline(pipe.unet)
    for v, o in zip(runs, outs):
        assert torch.equal(o, fresh.denoise(*inp, STEPS, GS, ap_scale=v, use_graph=False)), v
    assert len({o.cpu().numpy().tobytes() for o in outs}) == len(runs)  # four different results
    assert torch.equal(pipe.denoise(*inp, STEPS, GS, ap_scale=0.25), outs[0]) and (pipe.graph_captures, pipe.graph_hits) == (1, 4)
    (key,) = pipe._graphs
    assert key[-1] == ("ap_scale", 1) and _floats(key) == [GS]  # a marker and the column count; no scale value
    # the processors' ``scale`` is not part of what such a step bakes in
    with _scales(pipe.unet, 0.9):
        assert torch.equal(pipe.denoise(*inp, STEPS, GS, ap_scale=0.5), outs[1]) and pipe.graph_captures == 1


def test_per_clip_values_equal_the_two_scalar_runs(dev):
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    inp = _inputs(dev, dtype)
    s = 0.8
    both = pipe.denoise(*inp, STEPS, GS, ap_scale=[[0.0, s]])
    assert pipe._graphs and next(iter(pipe._graphs))[-1] == ("ap_scale", 2) and tuple(pipe.last_ap_scale.shape) == (3, 2)
    with _scales(pipe.unet, 0.0):
        zero = pipe.denoise(*inp, STEPS, GS, use_graph=False)
    with _scales(pipe.unet, s):
        full = pipe.denoise(*inp, STEPS, GS, use_graph=False)
    assert torch.equal(both[0], zero[0]) and torch.equal(both[1], full[1])
    assert not torch.equal(both[0], full[0]) and not torch.equal(both[1], zero[1])
    assert torch.equal(both, pipe.denoise(*inp, STEPS, GS, ap_scale=[[0.0, s]], use_graph=False))
    with pytest.raises(ValueError, match="^ap_scale holds 3 per-clip values"):
        pipe.denoise(*inp, STEPS, GS, ap_scale=[[0.0, s, 1.0]])


def test_without_the_keyword_nothing_changes(dev, monkeypatch):
    """ap_scale=None: only the non-_tab entry points run, the graph key is today's, and the result is the one computed through proc.scale; a
    constant table equals it bit for bit (what pins the table path to the reference)"""
    from ap_adapter_amd import _lib as L
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    inp = _inputs(dev, dtype)
    lib, tab_calls = L.lib(), []
    for op in ENTRY.values():
        monkeypatch.setattr(lib, op + "_tab", (lambda real: lambda *a: (tab_calls.append(1), real(*a))[1])(getattr(lib, op + "_tab")))
    plain = pipe.denoise(*inp, STEPS, GS)
    eager = pipe.denoise(*inp, STEPS, GS, use_graph=False)
    assert not tab_calls and pipe.last_ap_scale is None
    (key,) = pipe._graphs
    assert "ap_scale" not in str(key) and len(key) == 14
    hand = _hand_loop(pipe, dev, dtype, *inp, [0.5] * STEPS)
    assert torch.equal(plain, hand) and torch.equal(eager, hand)
    const = pipe.denoise(*inp, STEPS, GS, ap_scale=0.5)
    assert tab_calls and torch.equal(const, plain) and pipe.graph_captures == 2
    with pytest.raises(ValueError, match="^ap_scale needs an audio condition"):
        pipe.denoise(inp[0], inp[1][:, :8].contiguous(), inp[2], inp[3], STEPS, GS, ap_scale=0.5)


def test_editing_with_a_schedule_whose_head_is_not_read(dev):
    """strength = 0.5 and an edit_region: the entries before the start may be NaN; the kept region is the source, bit for bit; captured ==
    eager; a NaN inside the run is rejected on the host"""
    from test_gpu_edit import _call_kw
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    B, N = 2, 6
    _, ehs, ehs1, m1 = _inputs(dev, dtype)
    kw = _call_kw(ehs, ehs1, m1, B, N, GS)
    x0 = R(B, 8, 26, 16, seed=70, std=0.7).to(dev)
    k = pipe.scheduler.edit_start_index(N, 0.5)
    assert k == 3
    sched = [NAN] * k + [1.0, 0.5, 0.25]
    g = lambda: torch.Generator().manual_seed(11)
    out = pipe(source_latents=x0, strength=0.5, edit_region=(0.2, 0.6), generator=g(), ap_scale=sched, **kw).audios
    assert tuple(pipe.last_ap_scale.shape) == (N - k, 1) and pipe.last_ap_scale[:, 0].tolist() == [1.0, 0.5, 0.25]
    assert torch.equal(out[:, :, :5], x0[:, :, :5]) and torch.equal(out[:, :, 15:], x0[:, :, 15:])
    assert not bool((out[:, :, 5:15] == x0[:, :, 5:15]).any()) and bool(torch.isfinite(out).all())
    eager = pipe(source_latents=x0, strength=0.5, edit_region=(0.2, 0.6), generator=g(), ap_scale=sched, use_graph=False, **kw).audios
    assert torch.equal(out, eager)
    assert not torch.equal(out, pipe(source_latents=x0, strength=0.5, edit_region=(0.2, 0.6), generator=g(), ap_scale=[NAN] * k + [1.0] * 3, **kw).audios)
    with pytest.raises(ValueError, match="^ap_scale: every value"):
        pipe(source_latents=x0, strength=0.5, edit_region=(0.2, 0.6), generator=g(), ap_scale=[1.0] * 4 + [NAN, 1.0], **kw)


def test_inversion_round_trip_under_a_schedule(dev):
    """invert + denoise under one condition and ONE ap_scale schedule returns the source latents: the bar of
    tests/test_gpu_invert.py::test_fp32_round_trip_returns_the_source (1e-3) on the same grid without the keyword"""
    import ap_adapter_amd as A
    dtype = torch.float32
    pipe = _pipe(dev, dtype)
    N, gs, strength = 6, 3.0, 0.5
    cond = _inputs(dev, dtype)[1:]
    x0 = R(2, 8, 26, 16, seed=70, std=0.7).to(dev)
    k = pipe.scheduler.edit_start_index(N, strength)
    sched = [NAN] * k + [1.0, 0.6, 0.2]
    g = torch.Generator().manual_seed(5)
    z0 = torch.randn(x0.shape, generator=g)
    inv = pipe.invert(A.EditSource(x0=x0, z0=z0), *cond, N, gs, start=k, eta=1.0, generator=g, ap_scale=sched)
    out = pipe.denoise(None, *cond, N, gs, source=inv, start=k, eta=1.0, ap_scale=sched)
    err = rel_err(out, x0)
    print(f"\n[invert -> denoise under ap_scale={sched[k:]}, fp32 small UNet, N={N}, strength={strength}] rel err to the source {err:.3e}")
    assert all(("ap_scale", 1) in key for key in pipe._graphs) and len(pipe._graphs) == 2
    assert err < 1e-3
    other = pipe.denoise(None, *cond, N, gs, source=inv, start=k, eta=1.0, ap_scale=[NAN] * k + [0.2, 0.6, 1.0])
    assert rel_err(other, x0) > err  # another schedule in the edit pass does not retrace the source


def test_three_branch_run_with_a_per_clip_table(dev):
    from test_gpu_dual_guidance import _inputs3
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    inp = _inputs3(dev, dtype)
    tab = [[0.25, 1.0], [0.5, 0.5], [1.0, 0.0]]
    captured = pipe.denoise(*inp, STEPS, 3.0, audio_guidance_scale=2.0, ap_scale=tab)
    eager = pipe.denoise(*inp, STEPS, 3.0, audio_guidance_scale=2.0, ap_scale=tab, use_graph=False)
    assert torch.equal(captured, eager) and bool(torch.isfinite(captured).all()) and pipe.graph_captures == 1
    assert not torch.equal(captured, pipe.denoise(*inp, STEPS, 3.0, audio_guidance_scale=2.0, ap_scale=0.5))
    assert pipe.graph_captures == 2  # (one column instead of two: another key, still no value in it)
    assert all(_floats(k) == [] for k in pipe._graphs)

"""-m gpu: the audio prompt by region -- the three apad_*_qw entry points against their scalar twins bit for bit (a map entry v on a row equals
the scalar launch with s * v on that row; the table, the column modulo, the row stride, rejected arguments), the UNet with maps bound on every
decoupled processor, and the pipeline's ``ap_region=`` / ``ap_mask=`` keywords.

Nothing here has a tolerance except the inversion round trip (the bar of tests/test_gpu_invert.py): the map entry multiplies the scalar ONCE, in
fp32, and the product stands where the scalar stands in an expression the other suites pin, so every comparison is ``torch.equal``."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import nan_fill_free, rel_err

from test_gpu_ap_scale import ENTRY, GS, ROUTES, STEPS, R, _hand_loop, _inputs, _ip, _pipe, _precision, _scales, _table
from test_gpu_unet import _small_unet

pytestmark = pytest.mark.gpu
NAN = float("nan")
VALS = (0.0, 1.0, 0.5, 0.25, -1.5, 3.0)  # the map's values: off, on, fractions, a negative and an amplifying one
S = 0.55                                 # the descriptor's scale2
TAB = (0.25, 0.55, -1.5)                 # ... or one table value per column
QW_ROUTES = [r for r, v in ROUTES.items() if v[0] != "fused"]  # apad_fused_cross_attention has no per-query form


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    nan_fill_free(dev)


def f32mul(s, v):
    """the ONE fp32 multiply of the kernels, on the host"""
    return float(np.float32(s) * np.float32(v))


def _launcher(dev, route, B, N, La, Lt=8, seed=900):
    """random operands of one route on the device -> launch(scale2, query_weight) -> a NaN-prefilled output the launch wrote (the operands of
    test_gpu_ap_scale._launcher); La = 0 is the single-segment call"""
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
        def launch(scale2, qw=None):
            return ops.attention(x, k1, v1t, Lt, H, k2=k2, vt2=v2t, L2=La, scale2=scale2, out=out.fill_(NAN), query_weight=qw)
    elif op == "rows":
        wq_p, wo_p = ops.xrows_pack_weight(wq), ops.xrows_pack_weight(wo)

        def launch(scale2, qw=None):
            return ops.cross_attention_rows(x, wq_p, wo_p, bo, k1, v1t, H, ln=ln, k2=k2, vt2=v2t, scale2=scale2, out=out.fill_(NAN), query_weight=qw)
    else:
        wq_p, qb = ops.hs_pack_rows(wq, ln=ln)

        def launch(scale2, qw=None):
            return ops.hs_attention(x, wq_p, qb, self_attention=False, ln_eps=1e-5, k1=k1, vt1=v1t, k2=k2, vt2=v2t, scale2=scale2,
                                    out=out.fill_(NAN), query_weight=qw)
    return launch


def _cases():
    """the smallest shapes with a ragged last tile and more than one tile, in both segment-2 forms of each kernel"""
    out = []
    for route in QW_ROUTES:
        op = ROUTES[route][0]
        shapes = {"attention": [(100, 32), (100, 128)], "rows": [(40, 32), (128, 32), (40, 128)], "hs": [(40, 32), (64, 128)]}[op]
        out += [(route, n, la) for n, la in shapes]
    return out


def _value_index(cols, N):
    """[cols, N] indices into VALS: neighbouring tokens differ and the columns differ"""
    n, c = torch.arange(N)[None, :], torch.arange(cols)[:, None]
    return (n + 2 * c) % len(VALS)


def _map(dev, cols, N, ld=None, rows=None):
    """the fp32 map [rows or cols, ld or N] of _value_index; everything outside [cols, N] is NaN"""
    w = torch.full((rows or cols, ld or N), NAN)
    w[:cols, :N] = torch.tensor(VALS)[_value_index(cols, N)]
    return w.to(dev)


def _table_binding(dev):
    """a table whose read row (2 of 4) holds three different values and whose other rows are NaN"""
    from ap_adapter_amd import ops
    table = torch.full((4, 3), NAN, device=dev)
    table[2] = torch.tensor(TAB)
    return ops.Scale2Binding(table, torch.full((1,), 2, dtype=torch.int32, device=dev), 3)


def _assert_rows(out, scalar_of, cols, per_column_s, what):
    """every output row whose weight is v is the row of the scalar launch with s * v (s: the descriptor's, or the column's table entry)"""
    B, N = out.shape[:2]
    idx = _value_index(cols, N)
    for b in range(B):
        c = b % cols
        for i, v in enumerate(VALS):
            rows = (idx[c] == i).nonzero().flatten().to(out.device)
            assert rows.numel() > 0
            want = scalar_of[(c if per_column_s else None, v)]
            assert torch.equal(out[b][rows], want[b][rows]), (what, b, v)


@pytest.mark.parametrize("route,N,La", _cases())
def test_map_rows_equal_the_scalar_launches_bit_for_bit(dev, route, N, La):
    """B = 3 with cols = 3 and B = 6 on 3 columns: for each distinct map value v, the rows that carry it are the bits of the existing scalar entry
    point run with fp32(s) * fp32(v) -- with s from the descriptor, and from a table read at row 2 with one value per column"""
    from ap_adapter_amd import ops
    with _precision(ROUTES[route][3]):
        for B in (3, 6):
            launch = _launcher(dev, route, B, N, La)
            scalar_of = {(None, v): launch(f32mul(S, v)).clone() for v in VALS}
            scalar_of.update({(c, v): launch(f32mul(TAB[c], v)).clone() for c in range(3) for v in VALS})
            assert all(bool(torch.isfinite(t).all()) for t in scalar_of.values())
            for b in range(B):  # the weight matters, on every sample: any two different products give different rows
                runs = [scalar_of[(None, v)][b] for v in VALS]
                assert all(not torch.equal(runs[i], runs[j]) for i in range(len(VALS)) for j in range(i))
            qw = ops.QueryWeight(_map(dev, 3, N), 3)
            _assert_rows(launch(S, qw), scalar_of, 3, False, (route, B, "descriptor"))
            _assert_rows(launch(_table_binding(dev), qw), scalar_of, 3, True, (route, B, "table"))


@pytest.mark.parametrize("route,N,La", _cases())
def test_all_ones_map_is_the_launch_without_a_map(dev, route, N, La):
    """the whole tensor, with s from the descriptor and from the table; the same with ld > N and NaN in [N, ld) of every row (nothing past N is
    read into a result), and with cols = 1 broadcasting column 0 of a map whose other rows are NaN to every sample"""
    from ap_adapter_amd import ops
    with _precision(ROUTES[route][3]):
        launch = _launcher(dev, route, 3, N, La)
        plain, plain_tab = launch(S).clone(), launch(_table_binding(dev)).clone()
        assert bool(torch.isfinite(plain).all()) and not torch.equal(plain, plain_tab)
        ones = torch.ones(3, N, device=dev)
        assert torch.equal(launch(S, ops.QueryWeight(ones, 3)), plain)
        assert torch.equal(launch(_table_binding(dev), (ones, 3)), plain_tab)  # (a plain tuple is a QueryWeight too)
        wide = torch.full((3, N + 5), NAN, device=dev)
        wide[:, :N] = 1.0
        assert torch.equal(launch(S, ops.QueryWeight(wide, 3)), plain)
        # cols = 1: every sample reads column 0
        scalar_of = {(None, v): launch(f32mul(S, v)).clone() for v in VALS}
        _assert_rows(launch(S, ops.QueryWeight(_map(dev, 1, N, ld=N + 3, rows=3), 1)), scalar_of, 1, False, (route, "cols = 1"))


@pytest.mark.parametrize("route", ["attention-bf16", "attention-f32", "rows-bf16", "hs-bf16"])
def test_rejected_maps_are_errors_and_launch_nothing(dev, route, monkeypatch):
    """every rejected argument of the C ABI: refused by the wrapper (RuntimeError) and by the raw entry point (a negative code and a text naming
    it), the NaN-prefilled output untouched afterwards; one route per kernel (attention.hip's two, f32_ops.hip, hsattn.hip)"""
    from ap_adapter_amd import _lib as L, ops
    name = ENTRY[ROUTES[route][0]] + "_qw"
    lib = L.lib()
    real = getattr(lib, name)
    seen = []
    monkeypatch.setattr(lib, name, lambda d, t, w, s: (seen.append((d._obj, t._obj if t is not None else None, w._obj)), real(d, t, w, s))[1])
    N = 40
    with _precision(ROUTES[route][3]):
        launch, single = _launcher(dev, route, 3, N, 32), _launcher(dev, route, 3, N, 0)
        good = torch.full((3, N), 0.5, device=dev)
        done = launch(_table_binding(dev), ops.QueryWeight(good, 3))
        assert bool(torch.isfinite(done).all()) and len(seen) == 1
        desc, tab, qw = seen[0]
        untouched = lambda: bool(torch.isnan(done).all())
        for what, binding in {"a null map": (None, 3), "cols <= 0": (good, 0), "negative cols": (good, -2),
                              "ld < N": (good[:, :N - 1].contiguous(), 3)}.items():
            with pytest.raises(RuntimeError, match=name):
                launch(S, binding)
            assert untouched(), what
        with pytest.raises(RuntimeError, match=name + ".*second segment"):  # a map given to a single-segment call
            single(S, (good, 3))
        assert untouched()
        tb = _table_binding(dev)
        for what, t in {"a null table": (None, tb.step_ptr, 3), "rows <= 0": (torch.empty(0, 3, device=dev), tb.step_ptr, 3),
                        "table cols <= 0": (tb.table, tb.step_ptr, 0), "table ld < cols": (tb.table[:, :2].contiguous(), tb.step_ptr, 3)}.items():
            with pytest.raises(RuntimeError, match=name):
                launch(t, (good, 3))
            assert untouched(), what
        # what the wrapper checks itself: device, dtype, contiguity, shape (fewer map rows than columns would be read out of bounds)
        for what, binding in {"host map": (good.cpu(), 3), "fp64 map": (good.double(), 3), "strided map": (good.t(), 3), "1-D map": (good[0], 3),
                              "fewer rows than cols": (good[:2].contiguous(), 3)}.items():
            n = len(seen)
            with pytest.raises(RuntimeError):
                launch(S, binding)
            assert len(seen) == n and untouched(), what
        # the raw entry point, on the descriptor of the launch that worked
        monkeypatch.undo()
        done.fill_(NAN)

        def raw(t_change=None, null_t=False, null_w=False, **change):
            w = L.QueryWeight()
            for f, _ in L.QueryWeight._fields_:
                setattr(w, f, change.get(f, getattr(qw, f)))
            t = L.Scale2Tab()
            for f, _ in L.Scale2Tab._fields_:
                setattr(t, f, (t_change or {}).get(f, getattr(tab, f)))
            rc = real(C.byref(desc), None if null_t else C.byref(t), None if null_w else C.byref(w), None)
            text = lib.apad_last_error().decode()
            torch.cuda.synchronize()
            return rc, text

        bad = [dict(null_w=True), dict(w=None), dict(cols=0), dict(cols=-1), dict(ld=N - 1), dict(w=qw.w + 2)]
        bad += [dict(t_change=c) for c in (dict(table=None), dict(rows=0), dict(cols=0), dict(ld=2), dict(table=tab.table + 2))]
        for change in bad:
            rc, text = raw(**change)
            assert rc < 0 and text.startswith(name + ":") and untouched(), (change, rc, text)
        l2 = desc.L2
        desc.L2 = 0
        for null_t in (False, True):
            rc, text = raw(null_t=null_t)
            assert rc < 0 and text.startswith(name + ":") and untouched(), (null_t, rc, text)
        desc.L2 = l2
        rc, text = raw()  # and unchanged it still launches; so does a NULL table (the descriptor's scale2)
        assert rc == 0 and bool(torch.isfinite(done).all()), text
        done.fill_(NAN)
        rc, text = raw(null_t=True)
        assert rc == 0 and bool(torch.isfinite(done).all()), text


# ---------------------------------------------------------------------------------------------------------------------
# UNet level (small synthetic UNet, bf16)
# ---------------------------------------------------------------------------------------------------------------------
H_, W_ = 26, 16


def _maps(u, dev, mask):
    """{tokens: fp32 [cols, tokens] on the device} of a host mask [cols, 1, H, W]"""
    import ap_adapter_amd as A
    return {n: m.to(dev) for n, m in A.ap_mask_pyramid(mask, u.attention_grids(H_, W_)).items()}


def _forward_with(u, dev, dtype, x, cond, repeat, maps=None, cols=1, table=None):
    from test_gpu_dual_guidance import _forward
    if maps is not None:
        u.set_ap_token_weights(maps, cols)
    if table is not None:
        u.set_ap_scale_table(table, torch.ones(1, dtype=torch.int32, device=dev))
    try:
        return _forward(u, dev, dtype, x, cond, repeat)
    finally:
        u.clear_ap_token_weights()
        u.clear_ap_scale_table()


def _unet_case(dev, dtype=torch.bfloat16):
    u = _small_unet(dev, dtype)[0]
    u.requires_grad_(False)
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    x = lat.float().permute(0, 2, 3, 1).reshape(2, H_ * W_, 8).to(dtype).contiguous()
    return u, x, (ehs, ehs1, m1)


def test_unet_all_ones_binding_changes_nothing(dev, monkeypatch):
    """the fused routes off on both sides (a binding takes the 256-wide sites to the chain); every decoupled site goes through a _qw entry point"""
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd import processors as P
    import ap_adapter_amd as A
    monkeypatch.setattr(P, "USE_FUSED_XATTN", False)
    dtype = torch.bfloat16
    u, x, cond = _unet_case(dev, dtype)
    assert u.attention_grids(H_, W_) == [(13, 8), (7, 4), (4, 2)]
    lib, calls = L.lib(), {}
    for op in ("attention", "rows", "hs"):
        name = ENTRY[op] + "_qw"
        monkeypatch.setattr(lib, name, (lambda real, n: lambda *a: (calls.__setitem__(n, calls.get(n, 0) + 1), real(*a))[1])(getattr(lib, name), name))
    plain = _forward_with(u, dev, dtype, x, cond, 2)
    assert not calls and bool(torch.isfinite(plain).all())
    bound = _forward_with(u, dev, dtype, x, cond, 2, _maps(u, dev, torch.ones(1, 1, H_, W_)))
    assert torch.equal(bound, plain)
    assert sum(calls.values()) == len(A.ip_layer_names(u)) > 0, calls
    assert all(p.token_weights is None for p in _ip(u))
    half = torch.ones(1, 1, H_, W_)
    half[:, :, 5:15] = 0.0
    assert not torch.equal(_forward_with(u, dev, dtype, x, cond, 2, _maps(u, dev, half)), plain)  # a region matters


@pytest.mark.parametrize("repeat", [2, 3])
def test_unet_per_clip_constant_maps_equal_the_per_clip_table(dev, monkeypatch, repeat):
    """maps holding c_j everywhere on clip j, the processors' scale at 1: the forward under the ap_scale table [[c_0, c_1]], bit for bit, at
    batch_repeat = 2 and 3 (the guidance branches of a clip share its column); and table x map composes: table [[a, a]] under maps c_j / a"""
    from ap_adapter_amd import processors as P
    monkeypatch.setattr(P, "USE_FUSED_XATTN", False)
    dtype = torch.bfloat16
    u, x, cond = _unet_case(dev, dtype)
    if repeat == 3:
        from test_gpu_dual_guidance import _inputs3
        cond = _inputs3(dev, dtype)[1:]
    c = (0.125, 1.75)
    want = _forward_with(u, dev, dtype, x, cond, repeat, table=_table(dev, list(c)))
    mask = torch.tensor(c).reshape(2, 1, 1, 1).expand(2, 1, H_, W_)
    with _scales(u, 1.0):
        got = _forward_with(u, dev, dtype, x, cond, repeat, _maps(u, dev, mask), cols=2)
    assert got.shape[0] == 2 * repeat and torch.equal(got, want) and bool(torch.isfinite(got).all())
    a = 0.25  # exact quotients: 0.125 / 0.25 and 1.75 / 0.25
    both = _forward_with(u, dev, dtype, x, cond, repeat, _maps(u, dev, mask / a), cols=2, table=_table(dev, [a, a]))
    assert torch.equal(both, want)


def test_unet_binding_never_takes_the_fused_route(dev, monkeypatch):
    """the default routes with a binding: the recorded route of every decoupled site is not "fused", and without one it is what it was"""
    from ap_adapter_amd import processors as P
    dtype = torch.bfloat16
    u, x, cond = _unet_case(dev, dtype)
    seen = []
    real = P.route
    monkeypatch.setattr(P, "route", lambda kind, *a, **kw: (lambda r: (seen.append((kind, r, kw.get("query_weighted", False))), r)[1])(real(kind, *a, **kw)))
    _forward_with(u, dev, dtype, x, cond, 2)
    before = [(k, r) for k, r, _ in seen]
    assert not any(q for _, _, q in seen)
    seen.clear()
    _forward_with(u, dev, dtype, x, cond, 2, _maps(u, dev, torch.ones(1, 1, H_, W_)))
    dec = [(r, q) for k, r, q in seen if k == "decoupled"]
    assert dec and all(q and r != "fused" for r, q in dec)
    assert [(k, "chain" if (k, r) == ("decoupled", "fused") else r) for k, r in before] == [(k, r) for k, r, _ in seen]


def test_unet_binding_errors(dev):
    """a bound set without the call's token count, and a forward under autograd with maps bound: ValueErrors starting with ap_mask"""
    dtype = torch.bfloat16
    u, x, cond = _unet_case(dev, dtype)
    maps = _maps(u, dev, torch.ones(1, 1, H_, W_))
    with pytest.raises(ValueError, match="^ap_mask: no weight map is bound for a call of 104 tokens"):
        _forward_with(u, dev, dtype, x, cond, 2, {n: m for n, m in maps.items() if n != 104})
    # one decoupled site on its own, its adapter weights trainable: the training path has no per-token weight
    import ap_adapter_amd as A
    from ap_adapter_amd.unet import Attention
    attn = Attention(256, 768, 8, 32)
    proc = A.IPAttnProcessor2_0(hidden_size=256, name="site", cross_attention_dim=768, num_tokens=8, scale=0.5)
    attn.set_processor(proc)
    attn = attn.to(dev, dtype)
    hs, ehs = R(2, 40, 256).to(dev, dtype), R(2, 40, 768, seed=1).to(dev, dtype)
    proc.set_ap_token_weights({40: torch.ones(1, 40, device=dev)}, 1)
    with torch.enable_grad(), pytest.raises(ValueError, match="^ap_mask: the training path"):
        attn(hs, encoder_hidden_states=ehs)
    proc.clear_ap_token_weights()
    assert proc.token_weights is None


def test_full_geometry_rows_and_hs_sites_under_a_binding(dev, monkeypatch):
    """AudioLDM2-large geometry on a 2.56 s clip, bf16: with the 256-wide fused kernel out of the routes on BOTH sides, an all-ones binding changes
    no bit while the 384-wide sites run apad_cross_attention_rows_qw and the 640-wide ones apad_hs_attention_qw; per-clip constant maps equal
    the per-clip table; and on the default routes a binding moves exactly the fused sites to the chain"""
    import ap_adapter_amd as A
    from ap_adapter_amd import _lib as L, ops
    from ap_adapter_amd import processors as P
    from ap_adapter_amd.synthetic import synthetic_inputs
    from util import full_unet
    dtype, frames = torch.bfloat16, 64
    u = full_unet(0.55).to(dtype)
    u.requires_grad_(False)
    inp = synthetic_inputs(1, 32)
    ehs = A.AudioLDM2Pipeline(u).assemble_condition(inp["generated_prompt_embeds"], inp["audio_tokens"], inp["uncond_audio_tokens"], dtype)
    x = torch.cat([inp["latents"][:, :, :frames]] * 2).to(dtype).contiguous()
    u = u.to(dev)
    args = (x.to(dev), torch.tensor(501))
    kw = dict(encoder_hidden_states=ehs.to(dev), encoder_hidden_states_1=inp["prompt_embeds"].to(dtype).to(dev),
              encoder_attention_mask_1=inp["attention_mask"].to(dev), return_dict=False)
    grids = u.attention_grids(frames, 16)
    assert grids == [(32, 8), (16, 4), (8, 2)]
    lib, calls, routes = L.lib(), {}, []
    for op in ("attention", "rows", "hs"):
        name = ENTRY[op] + "_qw"
        monkeypatch.setattr(lib, name, (lambda real, n: lambda *a: (calls.__setitem__(n, calls.get(n, 0) + 1), real(*a))[1])(getattr(lib, name), name))
    real_route = P.route
    monkeypatch.setattr(P, "route", lambda kind, *a, **k: (lambda r: (routes.append((kind, r)), r)[1])(real_route(kind, *a, **k)))

    def run(mask=None, cols=1, table=None):
        with torch.no_grad():
            if mask is not None:
                u.set_ap_token_weights({n: m.to(dev) for n, m in A.ap_mask_pyramid(mask, grids).items()}, cols)
            if table is not None:
                u.set_ap_scale_table(table, torch.ones(1, dtype=torch.int32, device=dev))
            try:
                return u(*args, **kw)[0].clone()
            finally:
                u.clear_ap_token_weights()
                u.clear_ap_scale_table()

    default = run()
    default_routes = list(routes)
    assert ("decoupled", "fused") in default_routes and not calls
    routes.clear()
    run(torch.ones(1, 1, frames, 16))
    assert [(k, "chain" if (k, r) == ("decoupled", "fused") else r) for k, r in default_routes] == routes
    assert sum(calls.values()) == len(_ip(u)) == 32 and all(calls.get(ENTRY[op] + "_qw", 0) > 0 for op in ("attention", "rows", "hs")), calls
    monkeypatch.setattr(ops, "XATTN_C", 0)  # no width is the fused kernel's: its sites run the chain with or without a binding
    plain = run()
    assert bool(torch.isfinite(plain).all()) and bool(torch.isfinite(default).all())
    assert torch.equal(run(torch.ones(1, 1, frames, 16)), plain)
    c = (0.125, 1.75)  # (dyadic: the pooled levels of a constant mask hold the constant exactly)
    want = run(table=_table(dev, list(c)))
    with _scales(u, 1.0):
        got = run(torch.tensor(c).reshape(2, 1, 1, 1).expand(2, 1, frames, 16), cols=2)
    assert torch.equal(got, want) and not torch.equal(got, plain)


# ---------------------------------------------------------------------------------------------------------------------
# pipeline level (small synthetic UNet, 3 steps; 26 latent rows of 0.04 s)
# ---------------------------------------------------------------------------------------------------------------------
REGION, ROWS = (0.2, 0.6), (5, 15)


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_region_captured_equals_eager_and_regions_share_one_graph(dev, sampler):
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype, sampler)
    inp = _inputs(dev, dtype)
    captured = pipe.denoise(*inp, STEPS, GS, ap_region=REGION)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0)
    pyr = pipe.last_ap_mask
    assert sorted(pyr) == [8, 28, 104] and all(m.device.type == "cpu" and m.shape == (1, n) for n, m in pyr.items())
    eager = pipe.denoise(*inp, STEPS, GS, ap_region=REGION, use_graph=False)
    assert torch.equal(captured, eager) and bool(torch.isfinite(eager).all())
    # another region, and a mask of the same leading dimension, replay the SAME captured graph
    other = pipe.denoise(*inp, STEPS, GS, ap_region=(0.6, 1.0))
    mask = torch.zeros(1, 1, H_, W_)
    mask[:, :, :, 4:12] = 0.75  # a frequency band
    band = pipe.denoise(*inp, STEPS, GS, ap_mask=mask)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 2) and len(pipe._graphs) == 1
    (key,) = pipe._graphs
    assert key[-1] == ("ap_mask", 1) and len(key) == 15
    assert torch.equal(other, pipe.denoise(*inp, STEPS, GS, ap_region=(0.6, 1.0), use_graph=False))
    assert torch.equal(band, pipe.denoise(*inp, STEPS, GS, ap_mask=mask.numpy(), use_graph=False))
    assert len({o.cpu().numpy().tobytes() for o in (captured, other, band)}) == 3
    assert torch.equal(pipe.denoise(*inp, STEPS, GS, ap_region=REGION), captured) and pipe.graph_captures == 1
    assert all(p.token_weights is None for p in _ip(pipe.unet))  # the binding is gone after the call


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_mask_of_ones_equals_the_call_without_the_keyword(dev, sampler, monkeypatch):
    """the fused routes off on both sides; per-clip masks take one column per clip"""
    from ap_adapter_amd import processors as P
    monkeypatch.setattr(P, "USE_FUSED_XATTN", False)
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype, sampler)
    inp = _inputs(dev, dtype)
    plain = pipe.denoise(*inp, STEPS, GS)
    assert torch.equal(pipe.denoise(*inp, STEPS, GS, ap_mask=torch.ones(1, 1, H_, W_)), plain)
    assert torch.equal(pipe.denoise(*inp, STEPS, GS, ap_mask=np.ones((2, 1, 1, 1), np.float32)), plain)
    assert [k[-1] for k in pipe._graphs][1:] == [("ap_mask", 1), ("ap_mask", 2)]
    # clip 0 under ones, clip 1 under zeros: the rows of the two one-column runs
    per_clip = torch.tensor([1.0, 0.0]).reshape(2, 1, 1, 1)
    both = pipe.denoise(*inp, STEPS, GS, ap_mask=per_clip)
    zeros = pipe.denoise(*inp, STEPS, GS, ap_mask=torch.zeros(1, 1, H_, W_))
    assert torch.equal(both[0], plain[0]) and torch.equal(both[1], zeros[1]) and not torch.equal(both[1], plain[1])


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_region_with_a_schedule_equals_the_hand_loop(dev, sampler):
    """ap_region with ap_scale = [a, b, c]: the loop written out with the maps bound and every processor's ``scale`` set before each eager step"""
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype, sampler)
    inp = _inputs(dev, dtype)
    sched = [1.0, 0.5, 0.25]
    captured = pipe.denoise(*inp, STEPS, GS, ap_region=REGION, ap_scale=sched)
    eager = pipe.denoise(*inp, STEPS, GS, ap_region=REGION, ap_scale=sched, use_graph=False)
    (key,) = pipe._graphs
    assert key[-2:] == (("ap_scale", 1), ("ap_mask", 1))
    mask = torch.zeros(1, 1, H_, W_)
    mask[:, :, ROWS[0]:ROWS[1]] = 1.0
    pipe.unet.set_ap_token_weights(_maps(pipe.unet, dev, mask), 1)
    try:
        hand = _hand_loop(pipe, dev, dtype, *inp, sched)
    finally:
        pipe.unet.clear_ap_token_weights()
    assert torch.equal(captured, eager) and torch.equal(captured, hand) and bool(torch.isfinite(hand).all())
    assert not torch.equal(hand, _hand_loop(pipe, dev, dtype, *inp, sched))  # without the maps: another result


def test_without_the_keywords_nothing_changes(dev, monkeypatch):
    """no ap_region / ap_mask: none of the _qw entry points runs, the graph key is today's and the result is the hand loop's"""
    from ap_adapter_amd import _lib as L
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    inp = _inputs(dev, dtype)
    lib, qw_calls = L.lib(), []
    for op in ("attention", "rows", "hs"):
        name = ENTRY[op] + "_qw"
        monkeypatch.setattr(lib, name, (lambda real: lambda *a: (qw_calls.append(1), real(*a))[1])(getattr(lib, name)))
    plain = pipe.denoise(*inp, STEPS, GS)
    eager = pipe.denoise(*inp, STEPS, GS, use_graph=False)
    assert not qw_calls and pipe.last_ap_mask is None
    (key,) = pipe._graphs
    assert "ap_mask" not in str(key) and len(key) == 14
    hand = _hand_loop(pipe, dev, dtype, *inp, [0.5] * STEPS)
    assert torch.equal(plain, hand) and torch.equal(eager, hand)
    pipe.denoise(*inp, STEPS, GS, ap_region=REGION)
    assert qw_calls and pipe.graph_captures == 2
    with pytest.raises(ValueError, match="^ap_region needs an audio condition"):
        pipe.denoise(inp[0], inp[1][:, :8].contiguous(), inp[2], inp[3], STEPS, GS, ap_region=REGION)
    with pytest.raises(ValueError, match="^ap_mask and ap_region are both given"):
        pipe.denoise(*inp, STEPS, GS, ap_region=REGION, ap_mask=torch.ones(1, 1, H_, W_))


def test_edit_region_and_ap_region_together(dev):
    """``edit_region`` regenerates rows 5 .. 15 and ``ap_region`` weighs the audio prompt there only: the kept rows are the source bit for bit,
    captured == eager, and the region of the prompt matters"""
    from test_gpu_edit import _call_kw
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    B, N = 2, 6
    _, ehs, ehs1, m1 = _inputs(dev, dtype)
    kw = _call_kw(ehs, ehs1, m1, B, N, GS)
    x0 = R(B, 8, H_, W_, seed=70, std=0.7).to(dev)
    g = lambda: torch.Generator().manual_seed(11)
    out = pipe(source_latents=x0, strength=0.5, edit_region=REGION, ap_region=REGION, generator=g(), **kw).audios
    assert torch.equal(out[:, :, :5], x0[:, :, :5]) and torch.equal(out[:, :, 15:], x0[:, :, 15:]) and bool(torch.isfinite(out).all())
    eager = pipe(source_latents=x0, strength=0.5, edit_region=REGION, ap_region=REGION, generator=g(), use_graph=False, **kw).audios
    assert torch.equal(out, eager)
    assert not torch.equal(out, pipe(source_latents=x0, strength=0.5, edit_region=REGION, generator=g(), **kw).audios)
    with pytest.raises(ValueError, match="^ap_region="):
        pipe(source_latents=x0, strength=0.5, edit_region=REGION, ap_region=(0.5, 2.0), generator=g(), **kw)


def test_inversion_round_trip_under_a_region(dev):
    """invert + denoise under one condition and ONE ap_region returns the source latents: the bar of
    tests/test_gpu_invert.py::test_fp32_round_trip_returns_the_source (1e-3) on the same grid without the keyword"""
    import ap_adapter_amd as A
    dtype = torch.float32
    pipe = _pipe(dev, dtype)
    N, gs, strength = 6, 3.0, 0.5
    cond = _inputs(dev, dtype)[1:]
    x0 = R(2, 8, H_, W_, seed=70, std=0.7).to(dev)
    k = pipe.scheduler.edit_start_index(N, strength)
    g = torch.Generator().manual_seed(5)
    z0 = torch.randn(x0.shape, generator=g)
    inv = pipe.invert(A.EditSource(x0=x0, z0=z0), *cond, N, gs, start=k, eta=1.0, generator=g, ap_region=REGION)
    out = pipe.denoise(None, *cond, N, gs, source=inv, start=k, eta=1.0, ap_region=REGION)
    err = rel_err(out, x0)
    print(f"\n[invert -> denoise under ap_region={REGION}, fp32 small UNet, N={N}, strength={strength}] rel err to the source {err:.3e}")
    assert all(("ap_mask", 1) in key for key in pipe._graphs) and len(pipe._graphs) == 2
    assert err < 1e-3
    other = pipe.denoise(None, *cond, N, gs, source=inv, start=k, eta=1.0, ap_region=(0.6, 1.0))
    assert rel_err(other, x0) > err  # another region in the edit pass does not retrace the source

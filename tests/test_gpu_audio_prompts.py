"""-m gpu: several audio prompts per clip -- apad_attention_multi against the single-prompt entry points bit for bit wherever an identity exists
(no extra segment, a weightless prompt, a partition of the queries among the prompts, a clip inside and outside its batch), against an fp32
torch restatement within test_attention_decoupled's bound elsewhere, its rejected arguments, the UNet with prompts bound on every decoupled
processor, and the pipeline's ``audio_prompts=`` keyword.

Operands are those of tests/test_gpu_ap_scale.py::_launcher (B = 3 samples, 8 heads, 8 text keys); outputs are NaN-prefilled, tables hold NaN in
the rows that are not read and maps hold NaN outside [cols, N]."""
import collections
import ctypes as C

import pytest
import torch

from test_gpu_kernels import TOL, q, rel_err  # noqa: F401  (q: the storage rounding the restatement's operands went through)
from util import nan_fill_free

from audio_prompts_oracle import multi_prompt_attention, v_of_vt
from test_gpu_ap_region import H_, REGION, VALS, W_, f32mul
from test_gpu_ap_scale import GS, ROUTES, STEPS, R, _hand_loop, _inputs, _ip, _launcher, _pipe, _precision

pytestmark = pytest.mark.gpu
NAN = float("nan")
NAME = "apad_attention_multi"
HEADS, LT, B3 = 8, 8, 3
TAB = (0.25, 0.55, -1.5)

# name: (width C, N, prompt lengths).  short: three full query tiles plus a ragged one, a ragged key tail, every segment <= 64 keys; long and
# mixed: the long form (one segment above 64 keys takes every segment there)
CASES = {"short": (256, 100, (32, 32, 40)), "long": (256, 100, (128, 100)), "mixed": (256, 100, (32, 128)),
         "384-wide": (384, 40, (32, 32)), "640-wide": (640, 40, (128, 100))}
MODES = {"bf16": "attention-bf16", "f16": "attention-f16", "f32": "attention-f32", "f32-high": "attention-f32-high"}
SAME_FORM = [(c, m) for c in ("short", "long") for m in MODES]                   # where multi and single launches pick the same form
EVERY = SAME_FORM + [(c, m) for c in ("mixed", "384-wide", "640-wide") for m in ("bf16", "f16")]


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    nan_fill_free(dev)


class _Seen(Exception):
    pass


def _operands(dev, route, B, N, La, seed):
    """(x, k1, v1t, k2, v2t) as test_gpu_ap_scale._launcher builds them for one route: its launch is stopped at the op it would call"""
    from ap_adapter_amd import ops
    got = {}

    def stop(*a, **kw):
        got["a"], got["kw"] = a, kw
        raise _Seen

    with pytest.MonkeyPatch.context() as mp:
        for name in ("attention", "cross_attention_rows", "hs_attention"):
            mp.setattr(ops, name, stop)
        try:
            _launcher(dev, route, B, N, La, seed=seed)(0.0)
        except _Seen:
            pass
    a, kw = got["a"], got["kw"]
    op = ROUTES[route][0]
    x, k1, v1t = (a[0], a[1], a[2]) if op == "attention" else (a[0], a[4], a[5]) if op == "rows" else (a[0], kw["k1"], kw["vt1"])
    return x, k1, v1t, kw["k2"], kw["vt2"]


Setup = collections.namedtuple("Setup", "q k1 v1t prompts out dtype N")


def _setup(dev, case, mode, lengths=None, B=B3):
    """q, the text segment and one (k, vt, L) per prompt; prompt j's K / V come from _launcher's seed 900 + 20 j"""
    C_, N, lens = CASES[case]
    lens = lengths or lens
    route = MODES[mode] if C_ == 256 else ("rows-" if C_ == 384 else "hs-") + mode
    x, k1, v1t, _, _ = _operands(dev, route, B, N, lens[0], 900)
    prompts = [_operands(dev, route, B, N, L, 900 + 20 * j)[3:] + (L,) for j, L in enumerate(lens)]
    return Setup(x, k1, v1t, prompts, torch.empty_like(x), x.dtype, N)


def _single(S, j, scale2, qw=None):
    """the existing entry points (apad_attention / _tab / _qw) with prompt j as segment 2"""
    from ap_adapter_amd import ops
    k, vt, L = S.prompts[j]
    return ops.attention(S.q, S.k1, S.v1t, LT, HEADS, k2=k, vt2=vt, L2=L, scale2=scale2, query_weight=qw, out=S.out.fill_(NAN)).clone()


def _multi(S, specs):
    """apad_attention_multi: specs = [(prompt index, scale2, query weight), ...] in launch order"""
    from ap_adapter_amd import ops
    (j0, s0, w0), rest = specs[0], specs[1:]
    k, vt, L = S.prompts[j0]
    extra = [ops.AudioSegment(*S.prompts[j], s, w) for j, s, w in rest]
    return ops.attention(S.q, S.k1, S.v1t, LT, HEADS, k2=k, vt2=vt, L2=L, scale2=s0, query_weight=w0, extra=extra, out=S.out.fill_(NAN)).clone()


def _table(dev, values, rows=4, row=2):
    """a binding whose read row holds ``values`` (one per column) and whose other rows are NaN"""
    from ap_adapter_amd import ops
    t = torch.full((rows, len(values)), NAN, device=dev)
    t[row] = torch.tensor(values, dtype=torch.float32)
    return ops.Scale2Binding(t, torch.full((1,), row, dtype=torch.int32, device=dev), len(values))


def _map(dev, w):
    """a QueryWeight of the host map w [cols, N]; NaN everywhere outside [cols, N]"""
    from ap_adapter_amd import ops
    cols, N = w.shape
    full = torch.full((cols + 1, N + 3), NAN)
    full[:cols, :N] = w
    return ops.QueryWeight(full.to(dev), cols)


def _vals_map(cols, N, shift):
    n, c = torch.arange(N)[None, :], torch.arange(cols)[:, None]
    return torch.tensor(VALS)[(n + 2 * c + shift) % len(VALS)]


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", EVERY)
def test_no_extra_segment_is_the_existing_launch(dev, case, mode):
    """n_extra = 0 equals apad_attention, apad_attention_tab and apad_attention_qw (with and without a table) with the same d, t and w"""
    with _precision(ROUTES[MODES[mode]][3]):
        S = _setup(dev, case, mode)
        w = _map(dev, _vals_map(B3, S.N, 0))
        for s2, qw in ((0.55, None), (_table(dev, TAB), None), (0.55, w), (_table(dev, TAB), w)):
            want = _single(S, 0, s2, qw)
            assert bool(torch.isfinite(want).all())
            assert torch.equal(_multi(S, [(0, s2, qw)]), want), (case, mode, type(s2).__name__, qw is not None)


@pytest.mark.parametrize("case,mode", SAME_FORM)
def test_a_weightless_prompt_leaves_the_bits_of_the_launch_without_it(dev, case, mode):
    """two prompts, one of them at weight zero by a float 0.0, by a table entry 0 and by an all-zero map: the one-prompt launch of the other --
    elem(0 * a) is +-0 and t + +-0 == t (finite operands)"""
    with _precision(ROUTES[MODES[mode]][3]):
        S = _setup(dev, case, mode)
        zeros = {"float": (0.0, None), "table": (_table(dev, (0.0, -0.0, 0.0)), None), "map": (0.7, _map(dev, torch.zeros(B3, S.N)))}
        s, w = _table(dev, TAB), _map(dev, _vals_map(B3, S.N, 1))
        only0, only1 = _single(S, 0, s, w), _single(S, 1, s, w)
        assert bool(torch.isfinite(only0).all()) and bool(torch.isfinite(only1).all()) and not torch.equal(only0, only1)
        for how, (zs, zw) in zeros.items():
            assert torch.equal(_multi(S, [(0, s, w), (1, zs, zw)]), only0), (case, mode, how, "prompt 1 off")
            assert torch.equal(_multi(S, [(0, zs, zw), (1, s, w)]), only1), (case, mode, how, "prompt 0 off")


@pytest.mark.parametrize("case,mode", SAME_FORM)
def test_partitioned_rows_equal_the_scalar_launches_bit_for_bit(dev, case, mode):
    """three prompts; w_j[c][n] = 1 where (n + c) % 3 == j, else 0 (the columns rotated per clip); the scales a float, a table and a float, all
    different: row n of sample b is the row of the SCALAR single-prompt launch with prompt (n + b) % 3 under fp32(s) * fp32(1)"""
    with _precision(ROUTES[MODES[mode]][3]):
        lens = CASES[case][2] if case == "short" else CASES[case][2] + (70,)  # (a third long-form segment with a ragged tile)
        S = _setup(dev, case, mode, lens)
        n, c = torch.arange(S.N)[None, :], torch.arange(B3)[:, None]
        owner = (n + c) % 3  # [clip, query] -> prompt
        scales = [0.55, _table(dev, TAB), 1.25]
        out = _multi(S, [(j, scales[j], _map(dev, (owner == j).float())) for j in range(3)])
        assert bool(torch.isfinite(out).all())
        for b in range(B3):
            for j, s in enumerate((0.55, TAB[b], 1.25)):
                want = _single(S, j, f32mul(s, 1.0))
                rows = (owner[b] == j).nonzero().flatten().to(dev)
                assert rows.numel() >= S.N // 3 and torch.equal(out[b][rows], want[b][rows]), (case, mode, b, j)
                other = _single(S, (j + 1) % 3, f32mul(s, 1.0))
                assert not torch.equal(out[b][rows], other[b][rows])  # (the prompt matters)


@pytest.mark.parametrize("case,mode", SAME_FORM)
def test_a_clips_rows_do_not_depend_on_the_batch_around_it(dev, case, mode):
    """sample 1 alone, with its own K / V, table column and map column, and inside the batch of 3: the same rows"""
    from ap_adapter_amd import ops
    with _precision(ROUTES[MODES[mode]][3]):
        S = _setup(dev, case, mode)
        maps = [_vals_map(B3, S.N, 1 + j) for j in range(2)]
        tabs = [TAB, (1.25, -0.5, 0.75)]
        inside = _multi(S, [(j, _table(dev, tabs[j]), _map(dev, maps[j])) for j in range(2)])
        one = lambda t: t[1:2].contiguous()
        alone = Setup(one(S.q), one(S.k1), one(S.v1t), [(one(k), one(vt), L) for k, vt, L in S.prompts], torch.empty_like(one(S.q)), S.dtype, S.N)
        got = _multi(alone, [(j, _table(dev, tabs[j][1:2]), _map(dev, maps[j][1:2])) for j in range(2)])
        assert bool(torch.isfinite(inside).all()) and torch.equal(got[0], inside[1]), (case, mode)
        assert not torch.equal(inside[1], inside[0])


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: within test_attention_decoupled's bound of an fp32 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", EVERY)
def test_random_weights_and_maps_within_the_decoupled_bound(dev, case, mode):
    """every prompt under a random scale (a float, a table, a float, ...) and a random per-clip map drawn from test_gpu_ap_region.VALS, against
    text + sum_j s_j w_j softmax(q K_j^T / sqrt(d)) V_j in fp32 torch on the storage-rounded operands: rel_err < TOL[dtype].  Each case runs
    its prompts plus one more of its first length: four prompts on the short case, three elsewhere."""
    with _precision(ROUTES[MODES[mode]][3]):
        lens = CASES[case][2] + CASES[case][2][:1]
        S = _setup(dev, case, mode, lens)
        g = torch.Generator().manual_seed(77)
        specs, ref_prompts = [], []
        for j, (k, vt, L) in enumerate(S.prompts):
            s = (torch.rand(B3, generator=g) * 3 - 1.5).tolist()
            idx = torch.randint(0, len(VALS), (B3, S.N), generator=g)
            w = torch.tensor(VALS)[idx]
            if j % 2:
                specs.append((j, _table(dev, s), _map(dev, w)))
            else:
                s = [s[0]] * B3
                specs.append((j, s[0], _map(dev, w)))
            ref_prompts.append((k.float().cpu(), v_of_vt(vt.float().cpu(), L), torch.tensor(s, dtype=torch.float32), w))
        out = _multi(S, specs)
        ref = multi_prompt_attention(S.q.float().cpu(), S.k1.float().cpu(), v_of_vt(S.v1t.float().cpu(), LT), ref_prompts, HEADS)
        err = rel_err(out, ref)
        print(f"\n[{case}, {mode}, prompts {lens}] rel err to the fp32 restatement {err:.3e} (bound {TOL[S.dtype]:.0e})")
        assert bool(torch.isfinite(out).all()) and err < TOL[S.dtype], (case, mode, err)


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: rejected arguments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_rejected_arguments_are_errors_and_launch_nothing(dev, mode, monkeypatch):
    """every rejected argument of the C ABI: refused by the wrapper (RuntimeError naming the entry point) and by the raw entry point (a negative
    code and a text naming it), the NaN-prefilled output untouched afterwards"""
    from ap_adapter_amd import _lib as L, ops
    lib = L.lib()
    real = lib.apad_attention_multi
    seen = []

    def spy(d, t, w, xs, n, s):
        seen.append((d._obj, None if t is None else t._obj, None if w is None else w._obj, xs, n))
        return real(d, t, w, xs, n, s)

    monkeypatch.setattr(lib, NAME, spy)
    with _precision(ROUTES[MODES[mode]][3]):
        S = _setup(dev, "short", mode)
        N = S.N
        good_t, good_w = _table(dev, TAB), _map(dev, torch.ones(B3, N))
        seg = lambda j=1, **kw: ops.AudioSegment(*S.prompts[j], good_t, good_w)._replace(**kw)
        done = _multi(S, [(0, good_t, good_w), (1, good_t, good_w), (2, 0.5, None)])
        assert bool(torch.isfinite(done).all()) and len(seen) == 1
        untouched = lambda: bool(torch.isnan(S.out).all())

        def wrapper(extra, **kw):
            k, vt, Lk = S.prompts[0]
            args = dict(k2=k, vt2=vt, L2=Lk, scale2=good_t, query_weight=good_w)
            args.update(kw)
            return ops.attention(S.q, S.k1, S.v1t, LT, HEADS, extra=extra, out=S.out.fill_(NAN), **args)

        step = good_t.step_ptr
        k40, vt40 = S.prompts[2][:2]  # 40 keys, Lpad 64
        bad = {"four extras": [seg()] * 4, "L = 0": [seg(L=0)], "L < 0": [seg(L=-4)], "kv_batch_div = 0": [seg(kv_batch_div=0)],
               "kv_batch_div < 0": [seg(), seg(kv_batch_div=-1)], "null k": [seg(k=None)], "null vt": [seg(), seg(), seg(vt=None)],
               "Lpad < L": [seg(k=k40, vt=vt40[..., :32].contiguous(), L=40)], "Lpad % 32": [seg(k=k40, vt=vt40[..., :48].contiguous(), L=40)],
               "null table": [seg(scale2=(None, step, 3))], "rows <= 0": [seg(scale2=(torch.empty(0, 3, device=dev), step, 3))],
               "cols <= 0": [seg(scale2=(good_t.table, step, 0))], "ld < cols": [seg(scale2=(good_t.table[:, :2].contiguous(), step, 3))],
               "null map": [seg(query_weight=(None, 3))], "map cols <= 0": [seg(query_weight=(good_w.w, 0))],
               "map ld < N": [seg(query_weight=(good_w.w[:, :N - 1].contiguous(), 3))]}
        for what, extra in bad.items():
            with pytest.raises(RuntimeError, match=NAME):
                wrapper(extra)
            assert untouched(), what
        for what, kw in {"L2 == 0": dict(k2=None, vt2=None, L2=0, scale2=0.5, query_weight=None), "prompt 0: rows <= 0": dict(scale2=(torch.empty(0, 3, device=dev), step, 3)),
                         "prompt 0: map ld < N": dict(query_weight=(good_w.w[:, :N - 1].contiguous(), 3)), "prompt 0: null table": dict(scale2=(None, step, 3))}.items():
            for extra in ([seg()], []):
                with pytest.raises(RuntimeError, match=NAME):
                    wrapper(extra, **kw)
                assert untouched(), what
        # what the wrapper checks itself: device, dtype, contiguity, shape, the kind of the entries
        n = len(seen)
        k1_, vt1_, _ = S.prompts[1]
        for what, extra in {"host k": [seg(k=k1_.cpu())], "another dtype": [seg(k=k1_.double())], "strided vt": [seg(vt=vt1_.transpose(1, 2))],
                            "k of another width": [seg(k=k1_[..., :-8].contiguous())], "too few keys": [seg(L=k1_.shape[1] + 1)],
                            "not a segment": [(k1_, vt1_, 32)], "K/V samples short of the batch": [seg(k=k1_[:1], vt=vt1_[:1])],
                            "host table": [seg(scale2=(good_t.table.cpu(), step, 3))], "fp64 map": [seg(query_weight=(good_w.w.double(), 3))]}.items():
            with pytest.raises(RuntimeError):
                wrapper(extra)
            assert len(seen) == n and untouched(), what
        # the raw entry point, on the structs of the launch that worked
        monkeypatch.undo()
        desc, tab, qw, xs, n_extra = seen[0]
        assert n_extra == 2

        def raw(n=n_extra, extra=xs, t=tab, w=qw, d=None, x=None, x_tab=None, x_qw=None, j=1):
            keep = {}
            for f, v in (d or {}).items():
                keep[f] = getattr(desc, f)
                setattr(desc, f, v)
            ys = (L.AttnExtra * 3)()
            for i in range(n_extra):
                C.memmove(C.byref(ys[i]), C.byref(xs[i]), C.sizeof(L.AttnExtra))
            for f, v in (x or {}).items():
                setattr(ys[j], f, v)
            for f, v in (x_tab or {}).items():
                setattr(ys[0].tab, f, v)
            for f, v in (x_qw or {}).items():
                setattr(ys[0].qw, f, v)
            rc = real(C.byref(desc), None if t is None else C.byref(t), None if w is None else C.byref(w), None if extra is None else ys, n, None)
            text = lib.apad_last_error().decode()
            torch.cuda.synchronize()
            for f, v in keep.items():
                setattr(desc, f, v)
            return rc, text

        def changed(struct, **change):
            new = type(struct)()
            C.memmove(C.byref(new), C.byref(struct), C.sizeof(struct))
            for f, v in change.items():
                setattr(new, f, v)
            return new

        S.out.fill_(NAN)
        cases = [dict(n=-1), dict(n=4), dict(extra=None), dict(d=dict(L2=0)), dict(d=dict(lse=tab.table)), dict(n=0, d=dict(L2=0)),
                 dict(n=0, d=dict(lse=tab.table))]
        cases += [dict(x=c, j=j) for j in (0, 1) for c in (dict(L=0), dict(L=-1), dict(Lpad=0), dict(Lpad=16), dict(Lpad=48), dict(kv_batch_div=0),
                                                            dict(kv_batch_div=-2), dict(k=None), dict(vt=None))]
        cases += [dict(x_tab=c) for c in (dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-1), dict(ld=2), dict(table=tab.table + 2))]
        cases += [dict(x_qw=c) for c in (dict(cols=0), dict(cols=-1), dict(ld=N - 1), dict(w=qw.w + 2))]
        for n0 in (n_extra, 0):
            cases += [dict(n=n0, t=changed(tab, **c)) for c in (dict(table=None), dict(rows=0), dict(cols=0), dict(ld=2), dict(table=tab.table + 2))]
            cases += [dict(n=n0, w=changed(qw, **c)) for c in (dict(w=None), dict(cols=0), dict(ld=N - 1), dict(w=qw.w + 2))]
        for kw in cases:
            rc, text = raw(**kw)
            assert rc < 0 and NAME in text and untouched(), (kw, rc, text)
        rc, text = raw()  # and unchanged it still launches
        assert rc == 0 and torch.equal(S.out, done), text


# ---------------------------------------------------------------------------------------------------------------------
# UNet and pipeline (small synthetic UNet; 26 latent rows of 0.04 s; prompt 0 = the 32 audio tokens of _inputs, prompt 1 = 24 more)
# ---------------------------------------------------------------------------------------------------------------------
L0, L1_ = 32, 24
REGION_B = (0.6, 1.0)


def _more(ehs, n=L1_, seed=41, branches=2):
    """``n`` more audio tokens behind the condition: the zero-mel stand-in (one row set for the whole branch) on the first branch, recording
    tokens on the others"""
    rows = ehs.shape[0] // branches
    tok = R(rows, n, 768, seed=seed).to(ehs)
    unc = R(1, n, 768, seed=seed + 1).to(ehs).expand(rows, n, 768)
    return torch.cat([ehs, torch.cat([unc] + [tok] * (branches - 1))], dim=1).contiguous()


def _count_multi(monkeypatch):
    from ap_adapter_amd import _lib as L
    lib, calls = L.lib(), []
    monkeypatch.setattr(lib, NAME, (lambda real: lambda *a: (calls.append(a[4]), real(*a))[1])(lib.apad_attention_multi))
    return calls


def _chain_routes(monkeypatch):
    """processors.route answering "chain" for every decoupled site"""
    from ap_adapter_amd import processors as P
    real = P.route
    monkeypatch.setattr(P, "route", lambda kind, *a, **kw: "chain" if kind == "decoupled" else real(kind, *a, **kw))


def test_a_list_of_one_prompt_is_the_keyword_call(dev, monkeypatch):
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    inp = _inputs(dev, dtype)
    calls = _count_multi(monkeypatch)
    sched = [1.0, 0.5, 0.25]
    want = pipe.denoise(*inp, STEPS, GS, ap_scale=sched, ap_region=REGION)
    (key,) = pipe._graphs
    got = pipe.denoise(*inp, STEPS, GS, audio_prompts=[A.AudioPrompt(length=L0, ap_scale=sched, ap_region=REGION)])
    assert torch.equal(got, want) and bool(torch.isfinite(want).all())
    assert list(pipe._graphs) == [key] and (pipe.graph_captures, pipe.graph_hits) == (1, 1)
    again = pipe.denoise(*inp, STEPS, GS, audio_prompts=[A.AudioPrompt(length=L0, ap_scale=sched, ap_region=REGION)])
    assert torch.equal(again, want) and (pipe.graph_captures, pipe.graph_hits) == (1, 2)
    plain = pipe.denoise(*inp, STEPS, GS)
    assert torch.equal(pipe.denoise(*inp, STEPS, GS, audio_prompts=[A.AudioPrompt(length=L0)]), plain) and len(pipe._graphs) == 2
    assert not calls and pipe.last_audio_prompts is None


def test_a_weightless_second_prompt_leaves_no_trace(dev, monkeypatch):
    """two prompts with the second at ap_scale = 0.0: the one-prompt run with every decoupled site on the chain, bit for bit -- and the same
    bits under ANOTHER second recording"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    calls = _count_multi(monkeypatch)
    prompts = [A.AudioPrompt(length=L0), A.AudioPrompt(length=L1_, ap_scale=0.0)]
    two = pipe.denoise(lat, _more(ehs), ehs1, m1, STEPS, GS, audio_prompts=prompts)
    assert calls and set(calls) == {1} and bool(torch.isfinite(two).all())
    other = pipe.denoise(lat, _more(ehs, seed=43), ehs1, m1, STEPS, GS, audio_prompts=prompts)
    assert torch.equal(other, two) and (pipe.graph_captures, pipe.graph_hits) == (1, 1)
    heard = pipe.denoise(lat, _more(ehs), ehs1, m1, STEPS, GS, audio_prompts=[A.AudioPrompt(length=L0), A.AudioPrompt(length=L1_, ap_scale=0.5)])
    assert not torch.equal(heard, two)  # (with a weight the second recording matters)
    n = len(calls)
    _chain_routes(monkeypatch)
    one = pipe.denoise(lat, ehs, ehs1, m1, STEPS, GS)
    assert len(calls) == n and torch.equal(two, one)


def _bound_maps(pipe, dev, region):
    from ap_adapter_amd import ops
    mask = pipe.check_ap_mask(region, None, 2, H_, W_, has_audio=True)
    import ap_adapter_amd as A
    return {n: ops.QueryWeight(m.to(dev), 1) for n, m in A.ap_mask_pyramid(mask, pipe.unet.attention_grids(H_, W_)).items()}


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_two_prompts_captured_equals_eager_equals_the_hand_loop(dev, sampler):
    """prompt 0 under a per-step schedule in REGION, prompt 1 at a constant weight in another region: the captured step, the eager loop and a
    loop written out by hand on ``unet.set_audio_prompts`` (prompt 0 weighed by the processors' ``scale``, set before each step)"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype, sampler)
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    ehs2 = _more(ehs)
    sched = [1.0, 0.5, 0.25]
    prompts = [A.AudioPrompt(length=L0, ap_scale=sched, ap_region=REGION), A.AudioPrompt(length=L1_, ap_scale=0.8, ap_region=REGION_B)]
    captured = pipe.denoise(lat, ehs2, ehs1, m1, STEPS, GS, audio_prompts=prompts)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0)
    (key,) = pipe._graphs
    assert key[-1] == ("audio_prompts", (L0, L1_), (1, 1), (1, 1)) and len(key) == 15
    host = pipe.last_audio_prompts
    assert [p["length"] for p in host] == [L0, L1_] and torch.equal(host[0]["ap_scale"], torch.tensor(sched).reshape(3, 1))
    assert sorted(host[1]["ap_mask"]) == [8, 28, 104] and all(m.device.type == "cpu" for m in host[1]["ap_mask"].values())
    eager = pipe.denoise(lat, ehs2, ehs1, m1, STEPS, GS, audio_prompts=prompts, use_graph=False)
    pipe.unet.set_audio_prompts([L0, L1_], [None, 0.8], [_bound_maps(pipe, dev, REGION), _bound_maps(pipe, dev, REGION_B)])
    try:
        hand = _hand_loop(pipe, dev, dtype, lat, ehs2, ehs1, m1, sched)
        flat = _hand_loop(pipe, dev, dtype, lat, ehs2, ehs1, m1, [1.0, 1.0, 1.0])
    finally:
        pipe.unet.clear_audio_prompts()
    assert torch.equal(captured, eager) and torch.equal(captured, hand) and bool(torch.isfinite(hand).all())
    assert not torch.equal(hand, flat)  # the later steps' values are read
    assert all(p.audio_prompts is None and p.scale == 0.5 for p in _ip(pipe.unet)) and pipe.unet._ap_prompt_cols == ()


def test_other_recordings_regions_and_weights_replay_the_same_graph(dev, monkeypatch):
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    AP = A.AudioPrompt
    band = torch.zeros(1, 1, H_, W_)
    band[:, :, :, 4:12] = 0.75
    runs = [(_more(ehs), [AP(length=L0, ap_scale=[1.0, 0.5, 0.25], ap_region=REGION), AP(length=L1_, ap_scale=0.8, ap_region=REGION_B)]),
            (_more(ehs, seed=47), [AP(length=L0, ap_scale=0.3, ap_region=REGION_B), AP(length=L1_, ap_scale=[0.0, 0.5, 1.0], ap_mask=band)]),
            (_more(ehs.flip(0).contiguous(), seed=49), [AP(length=L0, ap_scale=-0.5, ap_mask=band.numpy()), AP(length=L1_, ap_scale=1.5, ap_region=REGION)])]
    outs = [pipe.denoise(lat, e, ehs1, m1, STEPS, GS, audio_prompts=p) for e, p in runs]
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 2) and len(pipe._graphs) == 1
    fresh = A.AudioLDM2Pipeline(pipe.unet)
    for (e, p), o in zip(runs, outs):
        assert torch.equal(o, fresh.denoise(lat, e, ehs1, m1, STEPS, GS, audio_prompts=p, use_graph=False))
    assert len({o.cpu().numpy().tobytes() for o in outs}) == 3
    # under two prompts no decoupled site takes a one-launch kernel; without the keyword the routes, the key and the entry points are today's
    from ap_adapter_amd import processors as P
    seen, real = [], P.route
    monkeypatch.setattr(P, "route", lambda kind, *a, **kw: (lambda r: (seen.append((kind, r, kw.get("multi", False))), r)[1])(real(kind, *a, **kw)))
    calls = _count_multi(monkeypatch)
    fresh.denoise(lat, ehs, ehs1, m1, STEPS, GS, use_graph=False)
    before = [(k, r) for k, r, _ in seen]
    assert not calls and not any(m for _, _, m in seen) and any(k == "decoupled" for k, _ in before)
    seen.clear()
    fresh.denoise(lat, runs[0][0], ehs1, m1, STEPS, GS, audio_prompts=runs[0][1], use_graph=False)
    dec = [(r, m) for k, r, m in seen if k == "decoupled"]
    assert dec and all(m and r == "chain" for r, m in dec) and len(calls) == len(dec)
    assert [(k, "chain" if k == "decoupled" else r) for k, r in before] == [(k, r) for k, r, _ in seen]
    n = len(calls)
    plain = pipe.denoise(lat, ehs, ehs1, m1, STEPS, GS)
    assert len(calls) == n and bool(torch.isfinite(plain).all())
    key = list(pipe._graphs)[-1]
    assert "audio_prompts" not in str(key) and len(key) == 14
    # both steps live in one cache: a replay of either refreshes the hoisted K / V of both, each with the split it was captured with
    monkeypatch.undo()
    captures = pipe.graph_captures
    assert torch.equal(pipe.denoise(lat, ehs, ehs1, m1, STEPS, GS), plain)
    for (e, p), o in zip(runs, outs):
        assert torch.equal(pipe.denoise(lat, e, ehs1, m1, STEPS, GS, audio_prompts=p), o)
    assert torch.equal(pipe.denoise(lat, ehs, ehs1, m1, STEPS, GS), plain) and pipe.graph_captures == captures
    # (last: the hand loop's own K / V hoist drops the cached steps' sets)
    assert torch.equal(plain, _hand_loop(pipe, dev, dtype, lat, ehs, ehs1, m1, [0.5] * STEPS))


def test_three_branches_with_two_prompts(dev):
    import ap_adapter_amd as A
    from test_gpu_dual_guidance import _inputs3
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    lat, ehs3, ehs1, m1 = _inputs3(dev, dtype)
    ehs3 = _more(ehs3, branches=3)
    prompts = [A.AudioPrompt(length=L0, ap_region=REGION), A.AudioPrompt(length=L1_, ap_scale=[[0.25, 1.0]], ap_region=REGION_B)]
    captured = pipe.denoise(lat, ehs3, ehs1, m1, STEPS, 3.0, audio_guidance_scale=2.0, audio_prompts=prompts)
    eager = pipe.denoise(lat, ehs3, ehs1, m1, STEPS, 3.0, audio_guidance_scale=2.0, audio_prompts=prompts, use_graph=False)
    assert torch.equal(captured, eager) and bool(torch.isfinite(captured).all()) and pipe.graph_captures == 1
    (key,) = pipe._graphs
    assert key[-1] == ("audio_prompts", (L0, L1_), (None, 2), (1, 1)) and "dual" in key


def test_inversion_round_trip_under_two_prompts(dev):
    """invert + denoise under one condition and ONE pair of prompts returns the source latents: the bar of
    test_gpu_ap_region.py::test_inversion_round_trip_under_a_region (1e-3)"""
    import ap_adapter_amd as A
    dtype = torch.float32
    pipe = _pipe(dev, dtype)
    N, gs, strength = 6, 3.0, 0.5
    _, ehs, ehs1, m1 = _inputs(dev, dtype)
    cond = (_more(ehs), ehs1, m1)
    x0 = R(2, 8, H_, W_, seed=70, std=0.7).to(dev)
    k = pipe.scheduler.edit_start_index(N, strength)
    prompts = [A.AudioPrompt(length=L0, ap_scale=[NAN] * k + [1.0, 0.6, 0.2], ap_region=REGION), A.AudioPrompt(length=L1_, ap_scale=0.8, ap_region=REGION_B)]
    g = torch.Generator().manual_seed(5)
    z0 = torch.randn(x0.shape, generator=g)
    inv = pipe.invert(A.EditSource(x0=x0, z0=z0), *cond, N, gs, start=k, eta=1.0, generator=g, audio_prompts=prompts)
    out = pipe.denoise(None, *cond, N, gs, source=inv, start=k, eta=1.0, audio_prompts=prompts)
    err = rel_err(out, x0)
    print(f"\n[invert -> denoise under two audio prompts, fp32 small UNet, N={N}, strength={strength}] rel err to the source {err:.3e}")
    assert all(k_[-1][0] == "audio_prompts" for k_ in pipe._graphs) and len(pipe._graphs) == 2
    assert err < 1e-3
    swapped = [A.AudioPrompt(length=L0, ap_scale=0.8, ap_region=REGION_B), A.AudioPrompt(length=L1_, ap_scale=0.2, ap_region=REGION)]
    assert rel_err(pipe.denoise(None, *cond, N, gs, source=inv, start=k, eta=1.0, audio_prompts=swapped), x0) > err


def test_a_forward_under_autograd_with_prompts_bound_raises(dev):
    import ap_adapter_amd as A
    from ap_adapter_amd.unet import Attention
    dtype = torch.bfloat16
    attn = Attention(256, 768, 8, 32)
    proc = A.IPAttnProcessor2_0(hidden_size=256, name="site", cross_attention_dim=768, num_tokens=8, scale=0.5)
    attn.set_processor(proc)
    attn = attn.to(dev, dtype)
    hs, ehs = R(2, 40, 256).to(dev, dtype), R(2, 8 + 32, 768, seed=1).to(dev, dtype)
    proc.set_audio_prompts([16, 16])
    with torch.enable_grad(), pytest.raises(ValueError, match="^audio_prompts: the training path"):
        attn(hs, encoder_hidden_states=ehs)
    with torch.no_grad(), pytest.raises(ValueError, match="^audio_prompts: the bound prompts hold"):
        attn(hs, encoder_hidden_states=ehs[:, :30].contiguous())
    with torch.no_grad():
        assert bool(torch.isfinite(attn(hs, encoder_hidden_states=ehs)).all())
    proc.clear_audio_prompts()
    assert proc.audio_prompts is None


def test_full_geometry_forward_under_two_prompts(dev, monkeypatch):
    """AudioLDM2-large geometry on a 2.56 s clip, bf16: two prompts with regions run every decoupled site -- 256-, 384- and 640-wide -- on the
    chain and the result is finite; with the second prompt at weight zero the forward is the one-prompt forward on the chain, bit for bit"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    from ap_adapter_amd import processors as P
    from ap_adapter_amd.synthetic import synthetic_inputs
    from util import full_unet
    dtype, frames = torch.bfloat16, 64
    u = full_unet(0.55).to(dtype)
    u.requires_grad_(False)
    inp = synthetic_inputs(1, 32)
    asm = A.AudioLDM2Pipeline(u).assemble_condition
    tok2 = R(1, 32, 768, seed=53).to(inp["audio_tokens"])
    ehs = asm(inp["generated_prompt_embeds"], inp["audio_tokens"], inp["uncond_audio_tokens"], dtype)
    ehs2 = asm(inp["generated_prompt_embeds"], [inp["audio_tokens"], tok2], inp["uncond_audio_tokens"], dtype)
    assert tuple(ehs2.shape) == (2, 8 + 64, 768) and torch.equal(ehs2[:, :40], ehs)
    x = torch.cat([inp["latents"][:, :, :frames]] * 2).to(dtype).contiguous()
    u = u.to(dev)
    args = (x.to(dev), torch.tensor(501))
    kw = dict(encoder_hidden_states_1=inp["prompt_embeds"].to(dtype).to(dev), encoder_attention_mask_1=inp["attention_mask"].to(dev), return_dict=False)
    grids = u.attention_grids(frames, 16)
    routes, real = [], P.route
    monkeypatch.setattr(P, "route", lambda kind, *a, **k: (lambda r: (routes.append((kind, r, a[0].to_q.weight.shape[0])), r)[1])(real(kind, *a, **k)))
    calls = _count_multi(monkeypatch)

    def run(cond, prompts=None):
        with torch.no_grad():
            if prompts is not None:
                u.set_audio_prompts(*prompts)
            try:
                return u(*args, encoder_hidden_states=cond.to(dev), **kw)[0].clone()
            finally:
                u.clear_audio_prompts()

    def maps(r0, r1):
        mask = torch.zeros(1, 1, frames, 16)
        mask[:, :, r0:r1] = 1.0
        return {n: ops.QueryWeight(m.to(dev), 1) for n, m in A.ap_mask_pyramid(mask, grids).items()}

    default = run(ehs)
    assert {(r, c) for k, r, c in routes if k == "decoupled"} == {("fused", 256), ("rows", 384), ("hs", 640)} and not calls
    routes.clear()
    both = run(ehs2, ([32, 32], [0.7, _table(dev, (0.9,))], [maps(0, 40), maps(24, 64)]))
    dec = [(r, c) for k, r, c in routes if k == "decoupled"]
    assert len(dec) == len(_ip(u)) == 32 == len(calls) and {r for r, _ in dec} == {"chain"} and {c for _, c in dec} == {256, 384, 640}
    assert bool(torch.isfinite(both).all()) and not torch.equal(both, default)
    off = run(ehs2, ([32, 32], [None, 0.0], None))
    off_tab = run(ehs2, ([32, 32], [None, _table(dev, (0.0,))], [None, maps(0, 64)]))
    monkeypatch.setattr(P, "route", lambda kind, *a, **k: "chain" if kind == "decoupled" else real(kind, *a, **k))
    n = len(calls)
    one = run(ehs)
    assert len(calls) == n and bool(torch.isfinite(one).all())
    assert torch.equal(off, one) and torch.equal(off_tab, one)

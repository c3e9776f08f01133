"""-m gpu: chroma features (apad_chroma) and chroma similarity (apad_chroma_similarity) against the independent fp64 restatement in
tests/chroma_oracle.py, and ``rank_by="chroma"`` through the pipeline.

Chroma bound (values in [0, 1], max-abs): 8 x the yardstick, floored at 2e-6, where the yardstick is the SAME oracle run in fp32 on the
CPU against its fp64 self on the same fp32 samples, measured inside the test.  The factor covers the kernel's radix-2 FFT with a
tabulated twiddle (about 11 roundings per bin; the CPU library's algorithm takes fewer); the floor covers the shortest clips, where
the yardstick is a handful of ulps.

Similarity bound, from the kernel's own order of operations (u = 2^-24; inputs are the same fp32 numbers on both sides):
  dot, |a|^2, |b|^2     12 fused multiply-adds over non-negative terms each           relative 12 u each
  sqrt sqrt * /         two roots (6 u + u each), their product (+ u), the quotient (+ u)   cosine: 12 u + 15 u + u = 28 u, cosine <= 1
  the mean              ceil(T / 256) - 1 serial adds per lane, 6 wave steps, 3 workgroup adds, one division: (ceil(T / 256) + 9) u
so |error| <= (37 + ceil(T / 256)) u: 2.3e-6 at T <= 256.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chroma_oracle as O
from util import nan_fill_free

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SMALL_N = (1, 511, 512, 2047, 2048, 5121)
SMALL_FRAMES = (1, 1, 2, 4, 5, 11)


def sim_bound(T):
    return (37 + math.ceil(T / 256)) * U


def nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def launch_chroma(clips, T, dev):
    """ops.chroma on a NaN-filled output: every element must be written"""
    from ap_adapter_amd import chroma, ops
    oh = torch.zeros(len(clips) + 1, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(c) for c in clips]), 0)
    packed = torch.from_numpy(np.concatenate(clips).astype(np.float32)).to(dev)
    out = nan(len(clips), T, 12, dev=dev)
    ops.chroma(packed, oh.to(dev), oh, *chroma.tables(dev), out)
    return out


def launch_similarity(a, b, idx, frames, dev, per_frame=True):
    from ap_adapter_amd import ops
    ih, fh = torch.tensor(idx, dtype=torch.int32), torch.tensor(frames, dtype=torch.int32)
    out = nan(a.shape[0], dev=dev)
    per = nan(a.shape[0], a.shape[1], dev=dev) if per_frame else None
    ops.chroma_similarity(a, b, ih.to(dev), ih, fh.to(dev), fh, out=out, per_frame=per)
    return out, per


def check_parity(clips, T, dev, what):
    out = launch_chroma(clips, T, dev).cpu()
    ref64 = O.chroma_batch(clips, T)
    yard = float((O.chroma_batch(clips, T, torch.float32).double() - ref64).abs().max())
    bound = max(8.0 * yard, 2e-6)
    err = float((out.double() - ref64).abs().max())
    print(f"{what}: fp32 CPU yardstick {yard:.3e}, bound {bound:.3e}, kernel max-abs error {err:.3e}")
    assert torch.isfinite(out).all()
    for b, c in enumerate(clips):
        assert bool((out[b, O.frame_count(len(c)):] == 0).all()), b  # rows past the clip's last frame
        assert float(out[b, : O.frame_count(len(c))].max()) == 1.0  # each frame divided by its own maximum
    assert err <= bound
    return out


def test_parity_small(dev):
    assert tuple(O.frame_count(n) for n in SMALL_N) == SMALL_FRAMES
    check_parity([O.signal(n, 10 + i) for i, n in enumerate(SMALL_N)], 12, dev, "small ragged batch")


def test_parity_real_size(dev):
    clips = [O.signal(163840, 20), O.signal(163840, 21)]
    assert O.frame_count(163840) == 321
    check_parity(clips, 321, dev, "2 x 163840 samples")


def test_silence(dev):
    tail = np.concatenate([O.signal(4096, 30), np.zeros(6000, np.float32)])
    out = launch_chroma([np.zeros(5121, np.float32), tail], 20, dev).cpu()
    assert bool((out[0] == 0).all())  # exactly 0, never NaN
    assert torch.isfinite(out).all()
    assert O.frame_count(len(tail)) == 20 and bool((out[1, 11:] == 0).all())  # frames 11.. start at sample 4608: all zeros
    assert bool((out[1, :10].max(dim=1).values == 1.0).all())  # frames that still reach the signal


@pytest.mark.parametrize("freq,row", [(440.0, 9), (261.63, 0), (329.63, 4)])
def test_pitch_anchors(dev, freq, row):
    out = launch_chroma([O.tone(freq).astype(np.float32)], 17, dev).cpu()
    assert (out[0].argmax(dim=1) == row).all() and float(out[0, :, row].min()) == 1.0


def test_batch_independence(dev):
    clips = [O.signal(n, 40 + i) for i, n in enumerate((5121, 700, 2048, 3000, 1))]
    whole = launch_chroma(clips, 12, dev)
    for b, c in enumerate(clips):
        assert torch.equal(launch_chroma([c], 12, dev)[0], whole[b]), b
    # the similarity of a candidate alone, and with other references around its own
    refs = launch_chroma([O.signal(5121, 50 + i) for i in range(3)], 12, dev)
    idx, frames = [2, 0, 1, 1, 0], [11, 2, 5, 6, 1]
    out, per = launch_similarity(whole, refs, idx, frames, dev)
    for i in range(5):
        o1, p1 = launch_similarity(whole[i:i + 1].contiguous(), refs, idx[i:i + 1], frames[i:i + 1], dev)
        o2, p2 = launch_similarity(whole[i:i + 1].contiguous(), refs[idx[i]:idx[i] + 1].contiguous(), [0], frames[i:i + 1], dev)
        assert torch.equal(o1[0], out[i]) and torch.equal(p1[0], per[i]) and torch.equal(o2[0], out[i]) and torch.equal(p2[0], per[i]), i


@pytest.mark.parametrize("T", [7, 300])
def test_similarity_against_the_oracle(dev, T):
    g = torch.Generator().manual_seed(60 + T)
    a, b = torch.rand(6, T, 12, generator=g), torch.rand(3, T, 12, generator=g)
    a[0, 1] = 0  # zero rows on either side: cosine 0 through the 1e-8 floor, never NaN
    b[2, 0] = 0
    a[4] = 0
    a[5] = b[1] * 0.5  # a scaled copy: cosine 1
    idx, frames = [2, 0, 1, 2, 0, 1], [T, 1, 0, T - 2, T, T]
    out, per = launch_similarity(a.to(dev), b.to(dev), idx, frames, dev)
    ref, ref_per = O.similarity(a, b, idx, frames)
    e, ep = float((out.cpu().double() - ref).abs().max()), float((per.cpu().double() - ref_per).abs().max())
    print(f"similarity T={T}: bound {sim_bound(T):.3e} (per frame {28 * U:.3e}), error {e:.3e}, per frame {ep:.3e}")
    assert sim_bound(T) < 1e-5
    assert e <= sim_bound(T) and ep <= 28 * U
    assert float(out[2]) == 0.0 and float(out[4]) == 0.0 and abs(float(out[5]) - 1.0) <= sim_bound(T)
    assert bool((per[1, 1:] == 0).all()) and bool((per[2] == 0).all()) and bool((per[3, T - 2:] == 0).all())
    # without the per-frame output the score is the same number
    assert torch.equal(launch_similarity(a.to(dev), b.to(dev), idx, frames, dev, per_frame=False)[0], out)


def test_refusals(dev):
    from ap_adapter_amd import chroma, ops
    tabs = chroma.tables(dev)
    x = torch.zeros(70000, device=dev)

    def run(offsets, T):
        oh = torch.tensor(offsets, dtype=torch.int64)
        return ops.chroma(x, oh.to(dev), oh, *tabs, nan(oh.numel() - 1, T, 12, dev=dev))

    with pytest.raises(RuntimeError, match="clip 1 is empty"):
        run([0, 600, 600, 900], 3)
    with pytest.raises(RuntimeError, match=r"offsets\[0\] must be 0"):
        run([4, 600], 3)
    with pytest.raises(RuntimeError, match="clip 1 has 3 frames, target_frames is 2"):
        run([0, 600, 1624], 2)
    with pytest.raises(RuntimeError, match="batch 65536 exceeds 65535"):
        run(list(range(65537)), 1)
    assert bool((run([0, 600, 1624], 3) == 0).all())  # the same operands, valid: silence
    a, b = torch.rand(2, 4, 12, device=dev), torch.rand(3, 4, 12, device=dev)
    for idx, frames, msg in (([0, 3], [4, 4], r"ref_index\[1\] = 3 outside \[0, 3\)"), ([-1, 0], [4, 4], r"ref_index\[0\] = -1 outside"),
                             ([0, 1], [4, 5], r"frames\[1\] = 5 outside \[0, 4\]"), ([0, 1], [-1, 4], r"frames\[0\] = -1 outside")):
        with pytest.raises(RuntimeError, match=msg):
            launch_similarity(a, b, idx, frames, dev)


def test_graph_capture(dev):
    """both launches recorded in one hipGraph and replayed on new contents of the same buffers equal eager, bit for bit"""
    from ap_adapter_amd import chroma, ops
    tabs = chroma.tables(dev)
    lens = (5121, 2048, 700)
    oh = torch.zeros(4, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor(lens), 0)
    od = oh.to(dev)
    ih, fh = torch.tensor([1, 0, 0], dtype=torch.int32), torch.tensor([5, 11, 2], dtype=torch.int32)
    idd, fd = ih.to(dev), fh.to(dev)
    first = torch.from_numpy(np.concatenate([O.signal(n, 70 + i) for i, n in enumerate(lens)])).to(dev)
    second = torch.from_numpy(np.concatenate([O.signal(n, 80 + i) for i, n in enumerate(lens)])).to(dev)
    x = first.clone()
    cg, sim, per = nan(3, 12, 12, dev=dev), nan(3, dev=dev), nan(3, 12, dev=dev)

    def both():
        ops.chroma(x, od, oh, *tabs, cg)
        ops.chroma_similarity(cg, cg, idd, ih, fd, fh, out=sim, per_frame=per)

    both()  # (loads the library and the tables outside the capture)
    cg_first = cg.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        both()
    x.copy_(second)
    for t in (cg, sim, per):
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (cg, sim, per)]
    for t in (cg, sim, per):
        t.fill_(float("nan"))
    both()
    torch.cuda.synchronize()
    for a, b in zip(got, (cg, sim, per)):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(got[0], cg_first)  # the replay read the buffers' new contents


def test_public_surface(dev):
    """chroma_stft / chroma_similarity: ragged lists, a rectangular GPU tensor, another sampling rate through frontend.resample"""
    import ap_adapter_amd as A
    clips = [O.signal(n, 90 + i) for i, n in enumerate((5121, 5121, 3000))]
    nan_fill_free(dev)
    rag = A.chroma_stft([torch.from_numpy(c) for c in clips])
    assert rag.shape == (3, 11, 12) and torch.equal(rag, launch_chroma(clips, 11, dev))
    rect = A.chroma_stft(torch.from_numpy(np.stack(clips[:2])).to(dev))
    assert torch.equal(rect, rag[:2])
    nan_fill_free(dev)
    sim, per = A.chroma_similarity(clips, clips[:1], return_per_frame=True)
    ref = O.waveform_similarity(clips, clips[:1])
    # chroma errors of both sides reach a cosine through at most |da| / |a| + |db| / |b| <= 2 sqrt(12) x the chroma bound (|a| >= 1)
    yard = float((O.chroma_batch(clips, 11, torch.float32).double() - O.chroma_batch(clips, 11)).abs().max())
    bound = sim_bound(11) + 2 * math.sqrt(12) * max(8.0 * yard, 2e-6)
    assert sim.shape == (3,) and per.shape == (3, 11) and float((sim.cpu().double() - ref).abs().max()) <= bound
    assert abs(float(sim[0]) - 1.0) <= sim_bound(11) and bool((per[2, 6:] == 0).all())  # 3000 samples: 6 frames in common
    x8 = torch.from_numpy(O.signal(4000, 95, sr=8000)).to(dev)
    up = A.frontend.resample(x8.reshape(1, -1), 8000, 16000)[0]
    assert torch.equal(A.chroma_stft(x8, sampling_rate=8000), A.chroma_stft(up))
    with pytest.raises(ValueError, match="references for 3 candidates"):
        A.chroma_similarity(clips, clips[:2])


# ---- through the pipeline: the small synthetic UNet, VAE and vocoder of the CLAP plumbing tests ----
SEED = 0
VOCODER_GAIN = 2.5
N, LEN = 3, int(0.64 * 16000)


def build_small(dev):
    import ap_adapter_amd as A
    import clap_audio_models as M
    from ap_adapter_amd import synthetic
    from text_models import CLAP_CFG, T5_CFG, PROMPTS, Tok, load_text_gold, ours_from_gold
    dtype = torch.float32
    R = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    unet = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    A.install_ap_adapter(unet, None, scale=0.5)
    synthetic.init_synthetic_(unet, 100, w_std=0.05, bias_std=0.02, norm_jitter=0.1)
    torch.manual_seed(3)
    vae = A.AutoencoderKL(A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8)).to(dev, dtype)
    voc = A.SpeechT5HifiGan(A.HifiGanConfig(upsample_initial_channel=256, upsample_rates=(5, 4, 2, 2, 2), upsample_kernel_sizes=(16, 16, 8, 4, 4)))
    # The plumbing tests' vocoder at its default initialisation attenuates its input layer by layer, so its biases set the output: every
    # latent comes out as the same waveform (a constant plus a fixed pattern at the Nyquist rate; the input-dependent part is 2 % of it), all
    # candidates score 1 - 1e-10 against any source, and no order can be decided.  The same module and seed with the weights x 2.5 and
    # the biases 0 passes its input on: the waveforms then differ and the scores of a group spread over about 3e-3.
    with torch.no_grad():
        for name, p in voc.named_parameters():
            p.mul_(VOCODER_GAIN) if name.endswith("weight") else p.zero_()
    voc = voc.to(dev, dtype)
    tg = load_text_gold()
    enc = A.PromptEncoder(ours_from_gold(tg, "clap2", "clap", dev, heads=2), ours_from_gold(tg, "t5", "t5", dev),
                          ours_from_gold(tg, "proj", "proj", dev), ours_from_gold(tg, "gpt2", "gpt2", dev))
    text = dict(prompt_encoder=enc, tokenizer=Tok(CLAP_CFG(2)["vocab_size"], CLAP_CFG(2)["pad_token_id"], 24, bos=0, eos=2),
                tokenizer_2=Tok(T5_CFG["vocab_size"], 0, 32, eos=1))
    clap = dict(audio_tower=M.ours(M.SMALL_CFG, M.SMALL_SEED).to(dev), feature_extractor=A.ClapFeatureExtractor(feature_size=16, max_length_s=2.5, truncation="rand_trunc"))
    P, Lt = len(PROMPTS), 8
    e = dict(prompt_embeds=R(P, 16, 1024, seed=20), negative_prompt_embeds=R(P, 16, 1024, seed=21),
             generated_prompt_embeds=R(P, Lt, 768, seed=22), negative_generated_prompt_embeds=R(P, Lt, 768, seed=23),
             attention_mask=torch.ones(P, 16, dtype=torch.long), negative_attention_mask=torch.ones(P, 16, dtype=torch.long))
    kw = dict(num_waveforms_per_prompt=N, num_inference_steps=2, audio_length_in_s=0.64, use_graph=False, output_type="pt", **e)
    return SimpleNamespace(unet=unet.to(dev, dtype), vae=vae, voc=voc, text=text, clap=clap, kw=kw, prompts=PROMPTS, P=P,
                           source=R(P, 8, 16, 16, seed=25))


@pytest.fixture(scope="module")
def small(dev):
    return build_small(dev)


def decoded_source(small):
    """the source latents through the same VAE and vocoder as the candidates"""
    scaling = getattr(getattr(small.vae, "config", None), "scaling_factor", 1.0)
    mel = small.vae.decode(small.source.to(small.unet.conv_in.weight.device) / scaling)
    mel = getattr(mel, "sample", mel)
    return small.voc(mel.squeeze(1) if mel.dim() == 4 else mel)[:, :LEN].float().cpu()


def _candidates_and_oracle(small):
    """a default call (the candidates as generated) and the oracle's similarities to the oracle-scored decoded source"""
    import ap_adapter_amd as A
    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)  # no towers, no tokenizers: the embeddings path
    kw = dict(source_latents=small.source, **small.kw)
    cand = pipe(generator=torch.Generator().manual_seed(SEED), **kw).audios
    assert cand.shape == (small.P * N, LEN) and not cand.is_cuda and pipe.last_chroma_similarity is None
    source = decoded_source(small)
    ref = O.waveform_similarity(list(cand.numpy()), list(source.numpy()))
    # the similarity bound, as for the kernel alone (the chromagrams' own fp32 error, 2.6e-7 measured, comes on top of the kernel's:
    # measured score error 7e-8 of the 2.3e-6)
    bound = sim_bound(21)
    return pipe, kw, cand, ref, bound


def test_pipeline_ranks_by_fidelity(dev, small):
    """The ranked call returns each prompt's candidates in the order of the ORACLE's similarities to the oracle-scored decoded source;
    that order is decided by gaps of at least 100 x the similarity bound and is not the identity (SEED chosen so: measured gap 6.6e-4
    against 2.3e-4, similarities 0.976 .. 0.984), and the pipeline's own scores agree with the oracle's within the bound."""
    pipe, kw, cand, ref, bound = _candidates_and_oracle(small)
    order = torch.argsort(ref.reshape(small.P, N), dim=1, descending=True)
    srt = torch.sort(ref.reshape(small.P, N), dim=1, descending=True).values
    gap = float((srt[:, :-1] - srt[:, 1:]).min())
    order = (order + torch.arange(small.P)[:, None] * N).reshape(-1)
    print(f"oracle similarities {ref.tolist()}; order {order.tolist()}; smallest deciding gap {gap:.3e}, 100 x bound {100 * bound:.3e}")
    assert gap >= 100 * bound
    assert order.tolist() != list(range(small.P * N))
    nan_fill_free(dev)
    out = pipe(generator=torch.Generator().manual_seed(SEED), rank_by="chroma", **kw).audios
    e = float((pipe.last_chroma_similarity.cpu().double() - ref).abs().max())
    print(f"last_chroma_similarity: error {e:.3e}, bound {bound:.3e}")
    assert e <= bound
    assert not out.is_cuda and torch.equal(out, cand[order])


def own_order(score):
    """each group of N by descending score, ties in generation order: written out, not through the product's helper"""
    return [i for p in range(len(score) // N) for i in sorted(range(p * N, (p + 1) * N), key=lambda j: (-score[j], j))]


def test_pipeline_scores_and_plumbing(dev, small):
    """around the ranked call: the returned order against the pipeline's own scores, the reference override, score_fidelity, the mixed
    form, the return types"""
    import ap_adapter_amd as A
    pipe, kw, cand, ref, bound = _candidates_and_oracle(small)
    gen = lambda: torch.Generator().manual_seed(SEED)
    nan_fill_free(dev)
    out = pipe(generator=gen(), rank_by="chroma", **kw).audios
    sim = pipe.last_chroma_similarity
    e = float((sim.cpu().double() - ref).abs().max())
    print(f"last_chroma_similarity {sim.tolist()}: error {e:.3e}, bound {bound:.3e}")
    assert sim.is_cuda and sim.dtype == torch.float32 and sim.shape == (small.P * N,) and e <= bound
    assert not out.is_cuda and torch.equal(out, cand[own_order(sim.cpu().double().tolist())])
    assert isinstance(pipe(generator=gen(), rank_by="chroma", **dict(kw, output_type="np")).audios, np.ndarray)
    # a given reference overrides the decoded source: against the first candidate of each group, that candidate scores 1
    given = cand[::N].clone()
    out2 = pipe(generator=gen(), rank_by="chroma", fidelity_reference=given, **kw).audios
    s2 = pipe.last_chroma_similarity.cpu()
    assert float((s2[::N] - 1.0).abs().max()) <= sim_bound(21) and torch.equal(out2, cand[own_order(s2.double().tolist())])
    assert float((s2.double() - O.waveform_similarity(list(cand.numpy()), list(given.numpy()))).abs().max()) <= bound
    s3 = pipe.score_fidelity(cand.to(dev), given.to(dev))  # score_fidelity alone
    assert torch.equal(s3.cpu(), s2) and pipe.last_chroma_similarity is s3
    # the mixed form: w_t cos_clap + w_f chroma within each prompt's group, the formula on the pipeline's own logits
    full = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc, **small.text, **small.clap)
    w_t, w_f = 1.0, 0.5
    out3 = full(generator=gen(), prompt=small.prompts, rank_by={"clap": w_t, "chroma": w_f}, **kw).audios
    logits, sim3 = full.last_logits_per_text.cpu().double(), full.last_chroma_similarity.cpu().double()
    assert logits.shape == (small.P, small.P * N) and torch.equal(sim3, sim.cpu().double())
    score = [w_t * float(logits[i // N, i]) / math.exp(full.logit_scale_t) + w_f * float(sim3[i]) for i in range(small.P * N)]
    assert own_order(score) != list(range(small.P * N))  # (the CLAP term decides here: the order is not the identity)
    assert torch.equal(out3, cand[own_order(score)])
    with pytest.raises(ValueError, match="needs one"):
        pipe(generator=gen(), rank_by="chroma", **small.kw)


def test_no_reach(dev, small, monkeypatch):
    """with ops.chroma out of order, a CLAP ranking call and a plain call run as before"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops

    def broken(*a, **k):
        raise AssertionError("ops.chroma reached without rank_by")

    monkeypatch.setattr(ops, "chroma", broken)
    monkeypatch.setattr(ops, "chroma_similarity", broken)
    full = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc, **small.text, **small.clap)
    gen = torch.Generator().manual_seed(SEED)
    ranked = full(generator=gen, prompt=small.prompts, **small.kw).audios
    assert ranked.shape == (small.P * N, LEN) and full.last_logits_per_text.shape == (small.P, small.P * N) and full.last_chroma_similarity is None
    ranked2 = full(generator=torch.Generator().manual_seed(SEED), prompt=small.prompts, rank_by="clap", **small.kw).audios
    assert torch.equal(ranked2, ranked)
    plain = full(generator=torch.Generator().manual_seed(SEED), **dict(small.kw, num_waveforms_per_prompt=1)).audios
    assert plain.shape == (small.P, LEN) and torch.isfinite(plain).all()
    edit = full(generator=torch.Generator().manual_seed(SEED), source_latents=small.source, strength=0.5, **small.kw).audios
    assert edit.shape == (small.P * N, LEN)
    with pytest.raises(AssertionError, match="reached"):
        full(generator=torch.Generator().manual_seed(SEED), source_latents=small.source, strength=0.5, rank_by="chroma", **small.kw)

"""-m gpu: the VAE log-mel front-end (apad_wav_stats + apad_stft_logmel behind frontend.wav_to_mel / wav_to_mel_batch) against
the fp64 restatement tests/vae_mel_oracle.py, and the trainer's wav-file path (CollateFunction -> train_batch) built on it.

Tolerances: 1e-4 absolute on the log-mel when kernel and oracle see the same 16 kHz samples (fp32 1024-point radix-2 FFT
and fp32 mel sums against float64; one log-mel unit is e), 2e-4 through the resampler, as in test_gpu_frontend.py."""
import math
import random
import wave

import numpy as np
import pytest
import torch

import vae_mel_oracle as O

pytestmark = pytest.mark.gpu

FLOOR = np.float32(np.log(np.float32(1e-5)))


def _signal(sr, seconds, seed, channels=1):
    n = int(round(sr * seconds))
    t = np.arange(n) / sr
    rs = np.random.RandomState(seed)
    out = []
    for c in range(channels):
        f = 150.0 + 5000.0 * t / max(t[-1], 1e-9)  # chirp plus noise plus DC
        out.append(0.35 * np.sin(2 * np.pi * (f * t / 2 + 100 * c * t)) + 0.05 * rs.randn(n) + 0.03)
    return np.stack(out)


def _write_wav(path, x, sr):
    """x float [channels, samples] in (-1, 1) -> 16-bit PCM; returns the decoded float32 samples (what torchaudio.load gives)"""
    pcm = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[0])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(pcm.T).tobytes())
    return pcm.astype(np.float32) / 32768.0


def _err(out, ref):
    out = out.float().cpu().numpy() if torch.is_tensor(out) else out
    assert np.isfinite(out).all()
    return float(np.abs(out.astype(np.float64) - ref).max())


@pytest.mark.parametrize("seconds,silent_half", [(10.0, False), (10.0, True), (3.0, False), (12.5, False)])
def test_kernel_vs_fp64_oracle_same_samples(dev, seconds, silent_half):
    from ap_adapter_amd import frontend as FE
    x = _signal(16000, seconds, 1)[0].astype(np.float32)
    if silent_half:
        x[x.size // 2:] = 0.0
    out = FE.wav_to_mel_batch([x], [16000], 10.0, device=dev)
    ref = O.mel_from_16k(x.astype(np.float64), 10.0)
    assert out.shape == (1, 1, 1024, 64) and out.dtype == torch.float32
    assert _err(out[0], ref) <= 1e-4


@pytest.mark.parametrize("sr,seconds,channels", [(16000, 10.0, 1), (16000, 3.0, 1), (16000, 12.5, 1), (44100, 12.5, 2),
                                                 (48000, 0.5, 1), (22050, 0.5, 2)])
def test_wav_to_mel_from_file_vs_oracle(dev, tmp_path, sr, seconds, channels):
    """wav file -> resample (channel 0) -> normalise over the whole clip -> pad -> STFT log-mel -> crop / zero rows"""
    from ap_adapter_amd import frontend as FE
    path = tmp_path / "clip.wav"
    decoded = _write_wav(path, _signal(sr, seconds, 2, channels) * 0.8, sr)
    out = FE.wav_to_mel(str(path), 10.0, device=dev)
    ref = O.wav_to_mel(decoded, sr, 10.0)
    assert out.shape == (1, 1024, 64) and out.dtype == torch.float32 and out.device.type == "cuda"
    assert _err(out, ref) <= 2e-4
    short = FE.wav_to_mel(str(path), 2.5, device=dev)  # another duration: target = int(2.5 * 102.4) = 256
    assert short.shape == (1, 256, 64) and _err(short, O.wav_to_mel(decoded, sr, 2.5)) <= 2e-4


@pytest.mark.parametrize("value", [0.0, 0.25])
def test_silent_and_constant_clip(dev, tmp_path, value):
    from ap_adapter_amd import frontend as FE
    path = tmp_path / "flat.wav"
    _write_wav(path, np.full((1, 3 * 16000), value), 16000)
    out = FE.wav_to_mel(str(path), 10.0, device=dev).cpu()
    assert not torch.isnan(out).any()
    v = out.reshape(-1)[0].item()
    assert torch.all(out == v)  # one value everywhere: logf(1e-5f)
    assert abs(v - float(FLOOR)) <= 2e-6


def test_ragged_batch_is_bit_equal_to_each_clip_alone(dev):
    from ap_adapter_amd import frontend as FE
    waves = [_signal(16000, 10.0, 3)[0], _signal(44100, 12.5, 4, 2), _signal(16000, 0.5, 5)[0], np.zeros(20000),
             _signal(22050, 3.3, 6)[0] * 0.1]
    srs = [16000, 44100, 16000, 16000, 22050]
    both = FE.wav_to_mel_batch(waves, srs, 10.0, device=dev)
    assert both.shape == (5, 1, 1024, 64)
    for i, (w, sr) in enumerate(zip(waves, srs)):
        assert torch.equal(both[i], FE.wav_to_mel_batch([w], [sr], 10.0, device=dev)[0]), i


def test_graph_capture_replays_bit_equal(dev):
    from ap_adapter_amd import frontend as FE
    clips = [torch.from_numpy(_signal(16000, s, 7 + i)[0].astype(np.float32)).to(dev) for i, s in enumerate((10.0, 4.0, 11.0))]
    packed = torch.cat(clips)
    oh = torch.tensor([0] + list(np.cumsum([c.numel() for c in clips])), dtype=torch.int64)
    off = oh.to(dev)
    stats = torch.empty(3, 2, device=dev)
    eager = torch.empty(3, 1, 1024, 64, device=dev)
    FE.logmel_launch(packed, off, oh, stats, eager, 1024 * 160, 1024)  # builds the tables outside the capture
    torch.cuda.synchronize()
    out = torch.full_like(eager, float("nan"))
    stats2 = torch.full_like(stats, float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        FE.logmel_launch(packed, off, oh, stats2, out, 1024 * 160, 1024)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(stats2, stats)
    assert torch.equal(eager, FE.wav_to_mel_batch([c.cpu().numpy() for c in clips], [16000] * 3, 10.0, device=dev))


def test_bad_input_is_an_error_not_a_fault(dev):
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd import frontend as FE
    with pytest.raises(ValueError):
        FE.wav_to_mel_batch([np.zeros(100, np.float32)], [16000], 10.0, device=dev)  # <= 100 samples
    with pytest.raises(ValueError):
        FE.wav_to_mel_batch([np.zeros(16000, np.float32)], [16000], 0.0, device=dev)  # target 0
    with pytest.raises(ValueError):
        FE.wav_to_mel_batch([np.zeros(16000, np.float32)], [16000], 0.03, device=dev)  # segment 480 <= 512
    with pytest.raises(NotImplementedError):
        FE.wav_to_mel("unused.wav", 10.0, snr=20.0)
    # the C entry points check their operands themselves
    x = torch.zeros(1000, device=dev)
    oh = torch.tensor([0, 60], dtype=torch.int64)
    off = oh.to(dev)
    stats = torch.zeros(1, 2, device=dev)
    out = torch.zeros(1, 16, 64, device=dev)
    window, tw, mel, rng = FE._logmel_tables(dev)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    assert lib.apad_wav_stats(x.data_ptr(), off.data_ptr(), oh.data_ptr(), stats.data_ptr(), 1, st) != 0
    assert b"100" in lib.apad_last_error()
    oh_ok = torch.tensor([0, 1000], dtype=torch.int64)
    args = lambda oh_, seg, tgt: (x.data_ptr(), off.data_ptr(), oh_.data_ptr(), stats.data_ptr(), window.data_ptr(), tw.data_ptr(),
                                  mel.data_ptr(), rng.data_ptr(), out.data_ptr(), 1, seg, tgt, st)
    assert lib.apad_stft_logmel(*args(oh, 16 * 160, 16)) != 0
    assert lib.apad_stft_logmel(*args(oh_ok, 512, 16)) != 0
    assert lib.apad_stft_logmel(*args(oh_ok, 16 * 160, 0)) != 0
    torch.cuda.synchronize()
    assert not out.any()  # nothing launched


def _collate_setup(dev, dtype=torch.float16):
    import ap_adapter_amd as A
    from ap_adapter_amd.synthetic import init_synthetic_
    mae = A.AudioMAEConditionCTPoolRand(depth=1)
    init_synthetic_(mae, 7, w_std=0.03, bias_std=0.02, norm_jitter=0.1)
    mae = mae.to(dev, dtype)
    enc = lambda texts: (torch.zeros(len(texts), 16, 1024, device=dev, dtype=dtype), torch.ones(len(texts), 16, device=dev),
                         torch.full((len(texts), 8, 768), 2.0, device=dev, dtype=dtype))
    return mae, enc


def _wav_examples(tmp_path):
    specs = [(16000, 10.0, 1), (44100, 12.5, 2), (22050, 3.0, 1)]
    ex, decoded = [], []
    for i, (sr, s, ch) in enumerate(specs):
        p = tmp_path / f"c{i}.wav"
        decoded.append((_write_wav(p, _signal(sr, s, 20 + i, ch) * 0.7, sr), sr))
        ex.append({"text": f"a recording of a {i}", "audio_path": str(p)})
    return ex, decoded


def test_collate_computes_the_vae_mel_from_audio_paths(dev, tmp_path):
    from ap_adapter_amd import frontend as FE
    from ap_adapter_amd import training as T
    mae, enc = _collate_setup(dev)
    ex, decoded = _wav_examples(tmp_path)
    b = T.CollateFunction(mae, enc, rng=random.Random(3), device=dev)(ex)
    assert b["mel"].shape == (3, 1, 1024, 64) and b["mel"].dtype == torch.float32
    for i, (w, sr) in enumerate(decoded):
        assert _err(b["mel"][i], O.wav_to_mel(w, sr, 10.0)) <= 2e-4, i
    # the AudioMAE condition is exactly what the fbank path gives for the same wavs and rng
    ref = T.CollateFunction(mae, enc, rng=random.Random(3), device=dev)(
        [{"text": e["text"], "fbank": FE.load_mel(e["audio_path"], device=dev)[0]} for e in ex])
    assert "mel" not in ref and b["pooling_rate"] == ref["pooling_rate"]
    assert torch.equal(b["generated_prompt_embeds"], ref["generated_prompt_embeds"])
    # precomputed mels: stacked as given; a mixed batch computes only the missing ones, in the 4-D layout
    pre = [torch.randn(1024, 64, device=dev) for _ in ex]
    same = T.CollateFunction(mae, enc, rng=random.Random(3), device=dev)([dict(e, mel=m) for e, m in zip(ex, pre)])
    assert torch.equal(same["mel"], torch.stack(pre))
    mixed = T.CollateFunction(mae, enc, rng=random.Random(3), device=dev)([dict(ex[0], mel=pre[0]), ex[1], ex[2]])
    assert mixed["mel"].shape == (3, 1, 1024, 64)
    assert torch.equal(mixed["mel"][0, 0], pre[0]) and torch.equal(mixed["mel"][1:], b["mel"][1:])
    # a shorter duration for the whole batch
    short = T.CollateFunction(mae, enc, rng=random.Random(3), device=dev, duration=2.5)(ex)
    assert short["mel"].shape == (3, 1, 256, 64)


def test_train_batch_from_wav_files_matches_a_hand_replay(dev, tmp_path):
    """CollateFunction on {"text", "audio_path"} -> train_batch: the same loss and gradient buffer as train_step replayed by
    hand from vae.encode(wav_to_mel_batch(...)) with the same device generator"""
    import ap_adapter_amd as A
    from ap_adapter_amd import frontend as FE
    from ap_adapter_amd import training as T
    from ap_adapter_amd.synthetic import init_synthetic_
    dtype = torch.bfloat16
    ucfg = A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16)

    def make():
        u = A.AudioLDM2UNet2DConditionModel(ucfg)
        A.install_ap_adapter(u, None, scale=0.5)
        init_synthetic_(u, 100, w_std=0.05, bias_std=0.02, norm_jitter=0.1)
        return A.AdapterTrainer(u.to(dev, dtype), lr=1e-3, gradient_accumulation_steps=4)

    vcfg = A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8)
    torch.manual_seed(13)
    vae = A.AutoencoderKL(vcfg)
    init_synthetic_(vae, 13, w_std=0.05, bias_std=0.02, norm_jitter=0.1)
    vae = vae.to(dev, dtype)
    mae, enc = _collate_setup(dev)
    ex, decoded = _wav_examples(tmp_path)
    ex, decoded = ex[:2], decoded[:2]
    batch = T.CollateFunction(mae, enc, rng=random.Random(5), device=dev)(ex)
    batch["generated_prompt_embeds"] = batch["generated_prompt_embeds"].to(dtype)
    batch["prompt_embeds"] = batch["prompt_embeds"].to(dtype)
    tr = make()
    loss = tr.train_batch(batch, vae, generator=torch.Generator(device=dev).manual_seed(7))
    g = torch.Generator(device=dev).manual_seed(7)
    mel = FE.wav_to_mel_batch([w for w, _ in decoded], [sr for _, sr in decoded], 10.0, device=dev)
    assert torch.equal(mel, batch["mel"])
    lat = vae.encode(mel).latent_dist.sample(generator=g, scale=vcfg.scaling_factor)
    assert lat.shape == (2, 8, 256, 16)
    noise = torch.randn(lat.shape, generator=g, device=dev, dtype=lat.dtype)
    t = torch.randint(0, 1000, (2,), generator=g, device=dev).long()
    tr2 = make()
    loss2 = tr2.train_step(lat, noise, t, batch["generated_prompt_embeds"], batch["prompt_embeds"], batch["attention_mask"].to(dev))
    assert math.isfinite(float(loss)) and float(loss) == float(loss2)
    assert torch.equal(tr.grad, tr2.grad) and float(tr.grad.abs().max()) > 0

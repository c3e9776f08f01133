"""CPU: the VAE log-mel front-end's host tables and its fp64 restatement (tests/vae_mel_oracle.py).  The STFT, Slaney mel
and log are pinned to torch.stft and transformers.audio_utils; the glue quirks of audioldm's read_wav_file / pad_wav /
_pad_spec (parity unpinned) are checked on the restatement itself."""
import numpy as np
import pytest
import torch

import vae_mel_oracle as O


def _clip(n, seed=0, sr=16000):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    f = 200.0 + 3000.0 * t / max(t[-1], 1e-9)  # chirp plus noise
    return 0.4 * np.sin(2 * np.pi * f * t) + 0.05 * rs.randn(n) + 0.02


def _transformers_mel():
    from transformers.audio_utils import mel_filter_bank
    return mel_filter_bank(513, 64, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T  # [64, 513]


def test_product_mel_table_matches_transformers():
    from ap_adapter_amd import frontend as FE
    ref = _transformers_mel()
    mel = FE.slaney_mel_filters()
    assert mel.shape == (64, 513) and mel.dtype == np.float32
    assert float(np.abs(mel - ref).max()) <= 1e-8  # one fp32 rounding of values <= 0.022
    window, tw, mel_t, rng = FE._logmel_tables(torch.device("cpu"))
    assert torch.equal(mel_t, torch.from_numpy(mel))
    for i in range(64):  # the kernel sums each filter over [lo, hi) only: that range holds every non-zero weight
        nz = np.nonzero(mel[i])[0]
        assert (int(rng[i, 0]), int(rng[i, 1])) == (nz[0], nz[-1] + 1)
    n = np.arange(1024)
    assert float(np.abs(window.numpy() - (0.5 - 0.5 * np.cos(2 * np.pi * n / 1024))).max()) < 1e-7  # periodic Hann
    k = np.arange(512)
    assert float(np.abs(tw.numpy() - np.stack([np.cos(2 * np.pi * k / 1024), -np.sin(2 * np.pi * k / 1024)], 1)).max()) < 1e-7


def test_oracle_mel_matches_transformers():
    assert float(np.abs(O.mel_filters() - _transformers_mel()).max()) < 1e-15


@pytest.mark.parametrize("n", [16000, 160 * 1024, 4321])
def test_oracle_stft_matches_torch_stft(n):
    y = O.normalize(_clip(n, 1))
    ref = torch.stft(torch.from_numpy(y), 1024, hop_length=160, win_length=1024, window=torch.hann_window(1024, periodic=True, dtype=torch.float64),
                     center=True, pad_mode="reflect", return_complex=True).abs().T.numpy()
    mag = O.stft_magnitude(y)
    assert mag.shape == ref.shape == (n // 160 + 1, 513)
    assert float(np.abs(mag - ref).max()) < 1e-10 * max(1.0, float(np.abs(ref).max()))


def test_oracle_log_mel_matches_transformers_spectrogram():
    from transformers.audio_utils import spectrogram, window_function
    y = O.normalize(_clip(3 * 16000, 2))
    ref = spectrogram(y, window_function(1024, "hann"), frame_length=1024, hop_length=160, fft_length=1024, power=1.0, center=True,
                      pad_mode="reflect", mel_filters=_transformers_mel().T, mel_floor=1e-5, log_mel="log").T
    out = O.log_mel(y)
    assert out.shape == ref.shape == (3 * 100 + 1, 64)
    assert float(np.abs(out - ref).max()) < 1e-6  # 3e-8 observed: both float64, different FFT order


def test_frame_count_and_crop():
    assert O.target_frames(10.0) == 1024 and O.target_frames(2.5) == 256 and O.target_frames(0.5) == 51
    for n in (1024 * 160, 1024 * 160 + 159, 1024 * 160 - 1):
        assert O.stft_magnitude(np.ones(n)).shape[0] == n // 160 + 1
    out = O.mel_from_16k(_clip(1024 * 160, 3), 10.0)
    assert out.shape == (1, 1024, 64)  # 1025 frames cropped to 1024
    full = O.log_mel(O.normalize(_clip(1024 * 160, 3)))
    assert full.shape[0] == 1025 and np.array_equal(out[0], full[:1024])
    short = O.pad_spec(full[:10], 16)
    assert short.shape == (16, 64) and not short[10:].any()  # zero-filled rows


def test_short_clip_is_zero_padded_at_the_waveform_level():
    x = _clip(3 * 16000, 4)
    out = O.mel_from_16k(x, 10.0)[0]
    y = np.concatenate([O.normalize(x), np.zeros(1024 * 160 - x.size)])
    assert np.array_equal(out, O.log_mel(y)[:1024])
    # frames well past the clip see only zeros: the floor, not zero rows
    assert np.all(out[400:] == np.log(1e-5))
    # a clip of 100 samples or fewer fails pad_wav's assert
    with pytest.raises(AssertionError):
        O.mel_from_16k(_clip(100, 5), 10.0)


def test_long_clip_is_not_truncated():
    """12.5 s at 10 s: the peak normalisation runs over the whole clip, and the last frames read real samples"""
    x = _clip(200000, 6)
    x[180000:] *= 4.0  # the loudest part lies past the 10 s segment
    out = O.mel_from_16k(x, 10.0)[0]
    trunc = O.mel_from_16k(x[:1024 * 160], 10.0)[0]
    assert out.shape == trunc.shape == (1024, 64)
    assert float(np.abs(out - trunc).max()) > 0.5  # normalised by the peak beyond the segment
    y = O.normalize(x)
    assert np.abs(y).max() == 0.5 and np.abs(y[:1024 * 160]).max() < 0.2
    assert np.array_equal(out, O.log_mel(y)[:1024])


@pytest.mark.parametrize("value", [0.0, 0.25])
def test_silent_and_constant_clip_give_the_floor(value):
    out = O.mel_from_16k(np.full(3 * 16000, value), 10.0)
    assert np.all(out == np.log(1e-5))


def test_sine_lands_in_its_mel_bin():
    f0 = 1500.0
    x = np.sin(2 * np.pi * f0 * np.arange(2 * 16000) / 16000)
    out = O.mel_from_16k(x, 2.0)[0]
    centre = O.mel_to_hz(np.linspace(O.hz_to_mel(0.0), O.hz_to_mel(8000.0), 66))[1:-1]
    peak = np.argmax(out[50:150].mean(0))
    assert abs(centre[peak] - f0) <= 0.5 * np.diff(centre)[peak - 1: peak + 1].max()


def test_wav_to_mel_rejects_what_it_does_not_implement():
    from ap_adapter_amd import frontend as FE
    for kw in (dict(augment_data=True), dict(mix_data=True), dict(snr=10.0)):
        with pytest.raises(NotImplementedError):
            FE.wav_to_mel("unused.wav", 10.0, **kw)
    with pytest.raises(ValueError):
        FE.wav_to_mel_batch([np.zeros(16000, np.float32)], [16000], duration=0.003)  # 320 samples <= the 512 reflect pad
    with pytest.raises(ValueError):
        FE.wav_to_mel_batch([np.zeros(16000, np.float32)], [16000, 16000])

"""CLAP log-mel features on the GPU: ``ClapFeatureExtractor`` with the constructor, attributes and call of transformers'
``ClapFeatureExtractor`` (models/clap/feature_extraction_clap.py) in its ``truncation="rand_trunc"`` form -- what
laion/clap-htsat-unfused and ``score_waveforms`` use -- on one HIP launch (``apad_clap_logmel``): resampling from the source rate,
the random crop of a long clip, the repeatpad / repeat / pad of a short one, the reflect-padded 1024-point STFT, the Slaney mel
projection and the dB scale.  Only the constant tables (window, twiddles, mel banks, polyphase kernel) and the crop starts are made
on the host.  The fusion variant (four stacked mels) is not on this path, as in clap_audio.py.
"""

import numpy as np
import torch

from . import _lib as L
from . import frontend, ops

PADDING_MODES = {"repeatpad": 0, "repeat": 1, "pad": 2}  # apad_clap_logmel's `padding`
_FFT = 1024


def source_index(i, n48, max_length, padding, start=0):
    """The index map of ``apad_clap_logmel``: which sample of the clip (n48 samples at the target rate) is sample ``i`` of the
    ``max_length`` samples that are framed -- or None where that sample is padding (zero).  ClapFeatureExtractor._get_input_mel:
    a longer clip is cropped at ``start``; a shorter one is tiled ``max_length // n48`` times and zero-padded (repeatpad), tiled
    and cut (repeat) or zero-padded (pad)."""
    if n48 > max_length:
        return start + i
    limit = {"repeatpad": (max_length // n48) * n48, "repeat": max_length, "pad": n48}[padding]
    return i % n48 if i < limit else None


def reflect_index(i, max_length):
    """np.pad(..., mode="reflect") of the ``max_length`` samples (the edge sample is not repeated): i in [-512, max_length + 512)
    -> [0, max_length), for max_length > 512"""
    if i < 0:
        i = -i
    if i >= max_length:
        i = 2 * (max_length - 1) - i
    return i


def _hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def _mel_to_hz_htk(m):
    return 700.0 * (np.power(10.0, np.asarray(m, np.float64) / 2595.0) - 1.0)


def htk_mel_filters(sr, n_fft, n_mels, fmin, fmax):
    """transformers.audio_utils.mel_filter_bank(norm=None, mel_scale="htk"): [n_fft / 2 + 1][n_mels] float64 (the fusion variant's
    filters; an attribute of the class, not used on this path)"""
    fft_f = np.linspace(0.0, sr // 2, n_fft // 2 + 1)
    mel_f = _mel_to_hz_htk(np.linspace(_hz_to_mel_htk(fmin), _hz_to_mel_htk(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    slopes = mel_f[None, :] - fft_f[:, None]
    return np.maximum(0.0, np.minimum(-slopes[:, :-2] / fdiff[:-1], slopes[:, 2:] / fdiff[1:]))


class ClapFeatures(dict):
    """what the call returns: ``input_features`` (GPU fp32 [B, 1, frames, feature_size]) and ``is_longer`` ([[bool]] per clip), as
    keys and as attributes like transformers' BatchFeature"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def clap_logmel_launch(packed, offsets, offsets_host, starts, starts_host, resampling, tables, out, max_length, hop, padding):
    """The launch on pre-allocated buffers (hipGraph-capturable: no allocation, no read-back).  packed fp32 [sum n] at the source
    rate, offsets int64 [B + 1] and starts int64 [B] on the device with their host copies (validation only), ``resampling`` =
    (kernel [new][kw] or None, width, orig, new), ``tables`` = ``ClapFeatureExtractor.tables(device)``, out fp32
    [B, 1, max_length // hop + 1, n_mels]."""
    kern, width, orig, new = resampling
    window, tw, mel, rng = tables
    B = offsets_host.numel() - 1
    L.check(L.lib().apad_clap_logmel(packed.data_ptr(), offsets.data_ptr(), offsets_host.data_ptr(), starts.data_ptr(), starts_host.data_ptr(),
                                     None if kern is None else kern.data_ptr(), orig, new, width, window.data_ptr(), tw.data_ptr(),
                                     mel.data_ptr(), rng.data_ptr(), out.data_ptr(), B, max_length, hop, out.shape[-1],
                                     PADDING_MODES[padding], ops._stream()), "apad_clap_logmel")
    return out


class ClapFeatureExtractor:
    model_input_names = ["input_features", "is_longer"]

    def __init__(self, feature_size=64, sampling_rate=48_000, hop_length=480, max_length_s=10, fft_window_size=1024, padding_value=0.0,
                 return_attention_mask=False, frequency_min=0, frequency_max=14_000, top_db=None, truncation="fusion", padding="repeatpad"):
        """transformers' names and defaults.  ``truncation`` and ``padding`` are resolved at the call, as there (the default
        "fusion" is stored and refused when a call resolves to it: construct with truncation="rand_trunc" as
        laion/clap-htsat-unfused does); ``top_db`` is stored and unused, as there."""
        if fft_window_size != _FFT:
            raise NotImplementedError(f"fft_window_size={fft_window_size}: apad_clap_logmel transforms 1024-sample windows")
        if not 1 <= feature_size <= 64:
            raise NotImplementedError(f"feature_size={feature_size}: apad_clap_logmel projects onto at most 64 mel filters")
        if return_attention_mask:
            raise NotImplementedError("return_attention_mask=True: the features carry no attention mask on this path")
        if padding_value != 0:
            raise NotImplementedError(f"padding_value={padding_value}: apad_clap_logmel pads with zeros")
        self.feature_size = feature_size
        self.sampling_rate = sampling_rate
        self.padding_value = padding_value
        self.padding_side = "right"
        self.return_attention_mask = return_attention_mask
        self.top_db = top_db
        self.truncation = truncation
        self.padding = padding
        self.fft_window_size = fft_window_size
        self.nb_frequency_bins = (fft_window_size >> 1) + 1
        self.hop_length = hop_length
        self.max_length_s = max_length_s
        self.nb_max_samples = max_length_s * sampling_rate
        self.frequency_min = frequency_min
        self.frequency_max = frequency_max
        self.mel_filters = htk_mel_filters(sampling_rate, fft_window_size, feature_size, frequency_min, frequency_max)
        self._mel = frontend.slaney_mel_filters(sr=sampling_rate, n_fft=fft_window_size, n_mels=feature_size, fmin=frequency_min,
                                                fmax=frequency_max)  # [feature_size][513] fp32: the kernel's operand
        self.mel_filters_slaney = self._mel.T.astype(np.float64)
        self._tables = {}

    def tables(self, dev):
        """(periodic Hann [1024], twiddles [512][2], Slaney mel [feature_size][513], each filter's non-zero bins [feature_size][2]
        int32) on ``dev``"""
        key = str(dev)
        if key not in self._tables:
            n = np.arange(_FFT, dtype=np.float64)
            window = (0.5 - 0.5 * np.cos(2 * np.pi * n / _FFT)).astype(np.float32)  # audio_utils.window_function(1024, "hann"), periodic
            k = np.arange(_FFT // 2, dtype=np.float64)
            tw = np.stack([np.cos(2 * np.pi * k / _FFT), -np.sin(2 * np.pi * k / _FFT)], axis=1).astype(np.float32)
            rng = np.zeros((self.feature_size, 2), np.int32)
            for i in range(self.feature_size):
                nz = np.nonzero(self._mel[i])[0]
                if nz.size:
                    rng[i] = (nz[0], nz[-1] + 1)
            self._tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (window, tw, self._mel, rng))
        return self._tables[key]

    @staticmethod
    def _resample_table(dev, source_rate, rate):
        """(kernel [new][kw] on ``dev`` or None, width, orig, new): ``frontend.resample``'s table, from its cache"""
        if int(source_rate) == int(rate):
            return None, 0, 1, 1
        key = ("rs", str(dev), int(source_rate), int(rate))
        if key not in frontend._tables:
            k, width, orig, new = frontend._resample_kernel(source_rate, rate)
            frontend._tables[key] = (torch.from_numpy(k).to(dev), width, orig, new)
        return frontend._tables[key]

    @staticmethod
    def _clips(raw_speech):
        """raw_speech -> (list of 1-D fp32 tensors, device): a GPU tensor [B, n] or [n], or a list of 1-D tensors / arrays (ragged)
        that is uploaded"""
        if torch.is_tensor(raw_speech) or isinstance(raw_speech, np.ndarray):
            t = torch.as_tensor(raw_speech)
            if t.dim() > 2:
                raise ValueError("Only mono-channel audio is supported for input to ClapFeatureExtractor")
            clips = [t] if t.dim() == 1 else list(t)
        elif isinstance(raw_speech, (list, tuple)) and len(raw_speech) and not isinstance(raw_speech[0], (float, int)):
            clips = [torch.as_tensor(np.asarray(c, dtype=np.float32) if not torch.is_tensor(c) else c) for c in raw_speech]
        else:
            clips = [torch.as_tensor(np.asarray(raw_speech, dtype=np.float32))]
        dev = next((c.device for c in clips if c.is_cuda), None)
        if dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("ClapFeatureExtractor: expected GPU waveforms (or a GPU to upload them to); the HIP path has no CPU fallback")
            dev = torch.device("cuda", torch.cuda.current_device())
        if any(c.dim() != 1 or c.numel() == 0 for c in clips):
            raise ValueError("ClapFeatureExtractor: every clip must be a non-empty 1-D waveform")
        return [c.to(device=dev, dtype=torch.float32) for c in clips], dev

    def __call__(self, raw_speech, truncation=None, padding=None, max_length=None, sampling_rate=None, return_tensors=None, *,
                 source_sampling_rate=None, crop_starts=None):
        """transformers' call, plus: ``source_sampling_rate`` = the rate the samples really have (default: ``sampling_rate``); the
        resampling to ``self.sampling_rate`` (``frontend.resample``'s polyphase kernel) then happens inside the launch.
        ``crop_starts`` = one entry per clip, the crop start (in samples at ``self.sampling_rate``) of each clip longer than
        ``max_length`` (None or 0 for the others); by default ``np.random.randint(0, overflow + 1)`` per long clip in batch order,
        the draws the installed extractor makes."""
        truncation = truncation if truncation is not None else self.truncation
        padding = padding if padding else self.padding
        if truncation != "rand_trunc":
            raise NotImplementedError(f"truncation={truncation!r}: only 'rand_trunc' is on the HIP path (the fusion variant of CLAP is not)")
        if padding not in PADDING_MODES:
            raise NotImplementedError(f"padding={padding!r}: one of {sorted(PADDING_MODES)}")
        if return_tensors not in (None, "pt"):
            raise NotImplementedError(f"return_tensors={return_tensors!r}: the features stay on the GPU as torch tensors")
        if sampling_rate is not None and sampling_rate != self.sampling_rate:
            raise ValueError(f"The model corresponding to this feature extractor: {self.__class__.__name__} was trained using a sampling rate of "
                             f"{self.sampling_rate}. Please make sure that the provided `raw_speech` input was sampled with "
                             f"{self.sampling_rate} and not {sampling_rate}.")
        max_length = int(max_length if max_length else self.nb_max_samples)
        if max_length <= _FFT // 2:
            raise ValueError(f"max_length {max_length} must exceed the {_FFT // 2}-sample reflect pad")
        clips, dev = self._clips(raw_speech)
        B = len(clips)
        source_rate = int(source_sampling_rate if source_sampling_rate is not None else self.sampling_rate)
        kern, width, orig, new = self._resample_table(dev, source_rate, int(self.sampling_rate))
        if crop_starts is not None and len(crop_starts) != B:
            raise ValueError(f"crop_starts: {len(crop_starts)} entries for {B} clips")
        starts_host = torch.zeros(B, dtype=torch.int64)
        is_longer = []
        for b, c in enumerate(clips):
            n48 = -(-c.numel() * new // orig)
            overflow = n48 - max_length
            given = None if crop_starts is None else crop_starts[b]
            if overflow > 0:
                start = int(np.random.randint(0, overflow + 1) if given is None else given)
                if not 0 <= start <= overflow:
                    raise ValueError(f"crop_starts[{b}] = {start} outside [0, {overflow}]")
                starts_host[b] = start
            elif given:
                raise ValueError(f"crop_starts[{b}] = {given}: clip {b} is not longer than max_length")
            is_longer.append([overflow > 0])
        offsets_host = torch.zeros(B + 1, dtype=torch.int64)
        offsets_host[1:] = torch.cumsum(torch.tensor([c.numel() for c in clips], dtype=torch.int64), 0)
        whole = torch.is_tensor(raw_speech) and raw_speech.is_cuda and raw_speech.dtype == torch.float32 and raw_speech.is_contiguous()
        packed = raw_speech.reshape(-1) if whole else torch.cat([c.contiguous() for c in clips])
        out = torch.empty(B, 1, max_length // self.hop_length + 1, self.feature_size, dtype=torch.float32, device=dev)
        clap_logmel_launch(packed, offsets_host.to(dev), offsets_host, starts_host.to(dev), starts_host,
                           (kern, width, orig, new), self.tables(dev), out, max_length, int(self.hop_length), padding)
        return ClapFeatures(input_features=out, is_longer=is_longer)

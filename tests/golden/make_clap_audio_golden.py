"""Writes tests/golden/clap_audio.safetensors: the OUTPUTS of the installed transformers ClapAudioModelWithProjection (CPU, fp32, seeded
weights -- tests/clap_audio_models.py) that the GPU tests compare the HIP tower with.  Weights and inputs are not stored (both sides
rebuild them from seeds); tests/test_clap_audio_host.py re-derives every entry from the installed module.

    python tests/golden/make_clap_audio_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def build():
    import clap_audio_models as M
    out = {}
    out["small.embeds"], out["small.pooler"] = M.oracle_outputs(M.SMALL_CFG, M.SMALL_SEED, M.SMALL_SHAPE)
    out["real.embeds"], out["real.pooler"] = M.oracle_outputs(M.REAL_CFG, M.REAL_SEED, M.REAL_SHAPE)
    out["pipe.logits"] = M.oracle_pipe_logits()
    return {k: v.contiguous() for k, v in out.items()}


if __name__ == "__main__":
    from safetensors.torch import save_file
    import clap_audio_models as M
    t = build()
    save_file(t, M.GOLD)
    print({k: tuple(v.shape) for k, v in t.items()}, os.path.getsize(M.GOLD), "bytes")
    print("pipe.logits", t["pipe.logits"])

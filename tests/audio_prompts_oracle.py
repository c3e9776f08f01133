"""fp32 torch restatement of the multi-prompt decoupled attention, on the host:

    out = A(q, K_text, V_text) + sum_j s_j[b] * w_j[b, n] * A(q, K_j, V_j),      A(q, K, V) = softmax(q K^T / sqrt(d)) V per head

every A an independently normalised softmax.  Operands are whatever the caller hands in (the GPU tests pass the storage-rounded device operands
converted to fp32).  No counterpart in the reference: this is attention_processor.py:429-454 with the audio branch repeated per prompt."""
import torch


def heads_of(t, heads):
    B, L, C = t.shape
    return t.reshape(B, L, heads, C // heads).transpose(1, 2)


def v_of_vt(vt, L):
    """[B, heads, d, Lpad] per-head transposed values -> [B, L, heads * d]"""
    B, H, d, _ = vt.shape
    return vt[..., :L].permute(0, 3, 1, 2).reshape(B, L, H * d)


def branch(q, k, v, heads):
    qh, kh, vh = (heads_of(t.float(), heads) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / qh.shape[-1] ** 0.5, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(q.shape)


def multi_prompt_attention(q, k_text, v_text, prompts, heads):
    """prompts: [(k [B, L, C], v [B, L, C], s: float or [B], w: None or [B, N])]"""
    out = branch(q, k_text, v_text, heads)
    B, N, _ = q.shape
    for k, v, s, w in prompts:
        sw = torch.as_tensor(s, dtype=torch.float32).reshape(-1, 1, 1).expand(B, 1, 1)
        if w is not None:
            sw = sw * w.float().reshape(B, N, 1)
        out = out + sw * branch(q, k, v, heads)
    return out

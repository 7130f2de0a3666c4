"""Torch restatements of the attention maps spe_forward_attention exports (csrc/attn_map.hip): what
nn.MultiheadAttention returns as output[1] with need_weights=True, the softmax probabilities averaged
over the heads.  Test infrastructure only."""
import torch
import torch.nn.functional as F

import model_ref


def head_avg_probs(q, k):
    """q [B,H,Tq,hd], k [B,H,Tk,hd] (per-head, after in_proj) -> [B,Tq,Tk] in q's dtype:
    mean_h softmax_j(q_h[i] / sqrt(hd) . k_h[j]), torch's order of operations (q scaled first)."""
    hd = q.shape[-1]
    s = (q * (hd ** -0.5)) @ k.transpose(-1, -2)
    return torch.softmax(s, dim=-1).mean(dim=1)


def head_avg_probs_folded(qf, k, nheads=8):
    """The bf16 decoder's folded cross-attention form (csrc/xattn.hip): qf [B,Tq,nheads*D] already scaled into
    the exp2 domain, one k [B,Tk,D] for every head -> [B,Tq,Tk]: mean_h softmax_j of 2^(qf_h[i] . k[j])."""
    B, Tq, _ = qf.shape
    D = k.shape[-1]
    s = qf.view(B, Tq, nheads, D).transpose(1, 2) @ k[:, None].transpose(-1, -2)      # [B,H,Tq,Tk]
    e = torch.exp2(s - s.amax(dim=-1, keepdim=True))
    return (e / e.sum(dim=-1, keepdim=True)).mean(dim=1)


def mha_weights_from_inputs(q_in, k_in, sd, p, nheads):
    """The head-averaged weights of the nn.MultiheadAttention at state_dict prefix `p` from its query /
    key inputs [B,L,d] (model_ref._mha's projections and head split, then head_avg_probs)."""
    W, b = sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"]
    d = W.shape[1]
    q = F.linear(q_in, W[:d], b[:d])
    k = F.linear(k_in, W[d:2 * d], b[d:2 * d])
    B, Lq, _ = q.shape
    q = q.view(B, Lq, nheads, d // nheads).transpose(1, 2)
    k = k.view(B, k.shape[1], nheads, d // nheads).transpose(1, 2)
    return head_avg_probs(q, k)


def oracle_attention_maps(images, sd, cfg, dtype=torch.float32):
    """Runs the oracle model (oracle/model_ref.py: its backbone, position table, attention, LayerNorm and
    head functions, in model_ref.forward's order) in `dtype` and captures, for every layer, the weights of
    encoder self_attn and decoder multihead_attn from the layer's inputs.
    Returns (outputs, enc_maps [list of [B,T,T]], dec_maps [list of [B,Q,T]]); outputs has pred_logits /
    pred_points.  In float32 the outputs are model_ref.forward's bit for bit (tests/test_attention_map.py)."""
    images = torch.as_tensor(images, dtype=torch.float32).to(dtype)
    sd = {k: torch.as_tensor(v, dtype=torch.float32).to(dtype) for k, v in sd.items()}
    nh = cfg.nheads
    _, _, neck = model_ref.backbone_s8(images, sd)
    B, _, h, w = neck.shape
    src = F.conv2d(neck, sd["input_proj.weight"], sd["input_proj.bias"])
    pos = model_ref.sine_pos(h, w, cfg.hidden_dim).to(dtype)[None].expand(B, -1, -1, -1)   # the model's fp32 table
    src = src.flatten(2).transpose(1, 2)
    pos = pos.flatten(2).transpose(1, 2)
    enc_maps, dec_maps = [], []
    for i in range(cfg.enc_layers):
        p = f"transformer.encoder.layers.{i}"
        qk = src + pos
        enc_maps.append(mha_weights_from_inputs(qk, qk, sd, p + ".self_attn", nh))
        src = model_ref._ln(src + model_ref._mha(qk, qk, src, sd, p + ".self_attn", nh), sd, p + ".norm1")
        ff = F.linear(F.relu(F.linear(src, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])),
                      sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])
        src = model_ref._ln(src + ff, sd, p + ".norm2")
    memory = src
    qpos = sd["query_embed.weight"][None].expand(B, -1, -1)
    tgt = torch.zeros_like(qpos)
    hs = []
    for i in range(cfg.dec_layers):
        p = f"transformer.decoder.layers.{i}"
        qk = tgt + qpos
        tgt = model_ref._ln(tgt + model_ref._mha(qk, qk, tgt, sd, p + ".self_attn", nh), sd, p + ".norm1")
        dec_maps.append(mha_weights_from_inputs(tgt + qpos, memory + pos, sd, p + ".multihead_attn", nh))
        tgt = model_ref._ln(tgt + model_ref._mha(tgt + qpos, memory + pos, memory, sd, p + ".multihead_attn", nh),
                            sd, p + ".norm2")
        ff = F.linear(F.relu(F.linear(tgt, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])),
                      sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])
        tgt = model_ref._ln(tgt + ff, sd, p + ".norm3")
        hs.append(model_ref._ln(tgt, sd, "transformer.decoder.norm"))
    hs = torch.stack(hs)
    out = {"pred_logits": F.linear(hs, sd["cls_embed.weight"], sd["cls_embed.bias"])[-1],
           "pred_points": model_ref._mlp3(hs, sd, "point_embed").sigmoid()[-1]}
    return out, enc_maps, dec_maps


def kernel_case(Tq, Tk, seed, B=2, H=8, hd=32, sigma=2.6):
    """Seeded q / k for the kernel test: N(0, sigma^2) entries, so the scaled scores q . k / sqrt(hd) are
    about N(0, sigma^4) (sigma 2.6: standard deviation 6.8, rows reach about +-20 and the row max matters)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Tq, hd, generator=g) * sigma
    k = torch.randn(B, H, Tk, hd, generator=g) * sigma
    return q, k


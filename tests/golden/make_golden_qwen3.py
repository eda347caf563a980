#!/usr/bin/env python
"""Golden vectors for the Qwen3 runtime: HF Qwen3ForCausalLM (fp32, eager attention, CPU) on the seeded tiny checkpoints of
tests/qwen3_ref.py.

    python tests/golden/make_golden_qwen3.py        # needs transformers

Configs, both head_dim 128, 4 layers, vocabulary 512: (A) hidden 256, 4 q / 2 kv heads (Hq * D != H), tied head; (B) hidden
256, 2 q / 2 kv heads, untied head.  A 40-token prompt.
Outputs: qwen3_logits.npz (full-prompt logits, last row), qwen3.json (prompt, 48 greedy tokens of HF generate, the arg-max
margin at each of them and, per config, what the restatement gives WITH THE TWO HEAD NORMS SWITCHED OFF: max abs logit
difference to HF, arg-max agreement over the prompt rows and the index of the first greedy token that differs).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import qwen3_ref as qr                                                  # noqa: E402


def hf_model(kind):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    c = dict(qr.CFGS[kind], **qr.COMMON)
    L = c["num_hidden_layers"]
    cfg = Qwen3Config(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                      num_hidden_layers=L, num_attention_heads=c["num_attention_heads"],
                      num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"], rms_norm_eps=c["rms_norm_eps"],
                      rope_parameters={"rope_type": "default", "rope_theta": c["rope_theta"]}, attention_bias=False,
                      use_sliding_window=False, layer_types=["full_attention"] * L,
                      tie_word_embeddings=c["tie_word_embeddings"], max_position_embeddings=40960,
                      attn_implementation="eager", bos_token_id=None, eos_token_id=None, pad_token_id=None)
    m = Qwen3ForCausalLM(cfg).eval()
    sd = qr.qwen3_state(kind)
    if c["tie_word_embeddings"]:
        sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "rotary" not in k], res
    return m


def greedy_ref(ref, prompt, n):
    seq = list(prompt)
    for _ in range(n):
        seq.append(int(ref.forward(seq)[-1].argmax()))
    return seq[len(prompt):]


@torch.no_grad()
def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(11)
    prompt = rs.randint(6, 512, size=40).tolist()
    out, npz = {"cfgs": qr.CFGS, "common": qr.COMMON, "seeds": qr.SEEDS, "prompt": prompt}, {}
    for kind in qr.CFGS:
        m = hf_model(kind)
        ids = torch.tensor([prompt])
        logits = m(ids).logits[0].float()
        npz[kind + "_logits"] = logits.numpy()
        npz[kind + "_logits_last"] = logits[-1].numpy()
        ref = qr.Qwen3Ref(kind).forward(prompt)
        out[kind + "_ref_vs_hf_max_abs"] = float((ref - logits).abs().max())
        g = m.generate(ids, max_new_tokens=48, do_sample=False, min_new_tokens=48)[0, len(prompt):].tolist()
        seq = prompt + g
        full = m(torch.tensor([seq])).logits[0].float()
        margins = []
        for i, tok in enumerate(g):
            row = full[len(prompt) + i - 1]
            top2 = row.topk(2).values
            assert int(row.argmax()) == tok
            margins.append(float(top2[0] - top2[1]))
        out[kind + "_greedy"] = g
        out[kind + "_margins"] = margins
        # the function a runtime WITHOUT the two head norms computes
        nn = qr.Qwen3Ref(kind, qk_norm=False)
        ln = nn.forward(prompt)
        gn = greedy_ref(nn, prompt, 48)
        first = next((i for i, (a, b) in enumerate(zip(gn, g)) if a != b), len(g))
        out[kind + "_nonorm_max_abs"] = float((ln - logits).abs().max())
        out[kind + "_nonorm_argmax_agreement"] = float((ln.argmax(-1) == logits.argmax(-1)).float().mean())
        out[kind + "_nonorm_first_diff"] = first
        out[kind + "_logit_max_abs"] = float(logits.abs().max())
        print(kind, "ref vs HF", out[kind + "_ref_vs_hf_max_abs"], "min margin", min(margins), "| logits max",
              out[kind + "_logit_max_abs"], "| no q/k norm: max abs", out[kind + "_nonorm_max_abs"], "arg-max agreement",
              out[kind + "_nonorm_argmax_agreement"], "first differing greedy token", first, "first margin < 0.1 at",
              next((i for i, x in enumerate(margins) if x < 0.1), len(margins)))
    np.savez_compressed(os.path.join(HERE, "qwen3_logits.npz"), **npz)
    with open(os.path.join(HERE, "qwen3.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Golden vectors for the Gemma-2 runtime: HF Gemma2ForCausalLM (fp32, eager attention, CPU) on the seeded tiny
checkpoints of tests/gemma2_ref.py.

    python tests/golden/make_golden_gemma2.py        # needs transformers

Configs: (A) head_dim 256, 4 q / 2 kv heads, 4 layers, sliding_window 16, caps 50 / 30, query_pre_attn_scalar 256;
(B) head_dim 128, query_pre_attn_scalar 144, window 16.  A 40-token prompt crosses the window.
Outputs: gemma2_logits.npz (full-prompt logits, last row), gemma2.json (prompt, 48 greedy tokens of HF generate and the
arg-max margin at each of them).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gemma2_ref as gr                                                 # noqa: E402


def hf_model(kind):
    from transformers import Gemma2Config, Gemma2ForCausalLM
    c = dict(gr.CFGS[kind], **gr.COMMON)
    L = c["num_hidden_layers"]
    cfg = Gemma2Config(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                       num_hidden_layers=L, num_attention_heads=c["num_attention_heads"],
                       num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"], rms_norm_eps=c["rms_norm_eps"],
                       rope_parameters={"rope_type": "default", "rope_theta": c["rope_theta"]},
                       query_pre_attn_scalar=c["query_pre_attn_scalar"], sliding_window=c["sliding_window"],
                       attn_logit_softcapping=c["attn_logit_softcapping"],
                       final_logit_softcapping=c["final_logit_softcapping"], hidden_activation="gelu_pytorch_tanh",
                       layer_types=["sliding_attention" if i % 2 == 0 else "full_attention" for i in range(L)],
                       tie_word_embeddings=True, max_position_embeddings=8192, attn_implementation="eager",
                       bos_token_id=None, eos_token_id=None, pad_token_id=None)
    m = Gemma2ForCausalLM(cfg).eval()
    sd = gr.gemma2_state(kind)
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "rotary" not in k], res
    return m


@torch.no_grad()
def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(11)
    prompt = rs.randint(6, 512, size=40).tolist()
    out, npz = {"cfgs": gr.CFGS, "common": gr.COMMON, "seeds": gr.SEEDS, "prompt": prompt}, {}
    for kind in gr.CFGS:
        m = hf_model(kind)
        ids = torch.tensor([prompt])
        logits = m(ids).logits[0].float()
        npz[kind + "_logits"] = logits.numpy()
        npz[kind + "_logits_last"] = logits[-1].numpy()
        ref = gr.Gemma2Ref(kind).forward(prompt)
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
        print(kind, "ref vs HF", out[kind + "_ref_vs_hf_max_abs"], "min margin", min(margins))
    np.savez_compressed(os.path.join(HERE, "gemma2_logits.npz"), **npz)
    with open(os.path.join(HERE, "gemma2.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

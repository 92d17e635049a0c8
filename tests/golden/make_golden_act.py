"""Generates tests/golden/tiny_act.npz: one training step of THE REFERENCE's own modules on the
tiny_act workload (workloads.tiny_act_config) for each activation of NAMES, the brain encoder's fc
stack built with encoder_fc_activation_function=<name> (reference create_fully_connected indexes
transformers' ACT2FN with it). Like make_golden.py it runs only where the reference is installed;
the tests read the .npz alone.

The file holds the inputs once and, per name, loss, logits, the gradient norm of every parameter
and the full gradients of the fc Linear parameters only (the GRU layer-0 weight gradient alone is
~690 KB; its norm stands for it), so the file stays well under 1 MB.

usage: python tests/golden/make_golden_act.py   (from the repo root)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from tests.golden import make_golden as mg  # noqa: E402
from wav2vec2forbrain_amd.util.init import deterministic_state  # noqa: E402
from wav2vec2forbrain_amd.workloads import make_batch, tiny_act_config  # noqa: E402

NAMES = ["relu", "relu2", "relu6", "tanh", "sigmoid", "mish", "quick_gelu", "laplace", "gelu_new", "gelu_10", "linear"]


def build_reference_model(cfg, tfw, bfe, w2v, base_args):
    """make_golden.build_reference_model with the fc activation of the workload."""
    name = "golden/" + cfg["name"]
    base_args.PRETRAINED_LATENT_SIZES[name] = cfg["hidden_size"]
    bfe.PRETRAINED_LATENT_SIZES[name] = cfg["hidden_size"]
    hf = tfw.Wav2Vec2Config(
        hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
        intermediate_size=cfg["ffn"], hidden_act="gelu", hidden_dropout=0.0, activation_dropout=0.0,
        attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0,
        num_conv_pos_embeddings=cfg["pos_k"], num_conv_pos_embedding_groups=cfg["pos_groups"], vocab_size=32,
        do_stable_layer_norm=False)
    hf._attn_implementation = "eager"

    def fake_from_pretrained(ckpt, **kw):
        c = tfw.Wav2Vec2Config.from_dict(hf.to_dict())
        for k, v in kw.items():
            setattr(c, k, v)
        c._attn_implementation = "eager"
        return c

    w2v.Wav2Vec2Config.from_pretrained = staticmethod(fake_from_pretrained)
    args = bfe.B2P2TBrainFeatureExtractorArgsModel(
        encoder_gru_hidden_size=cfg["gru_hidden"], encoder_num_gru_layers=cfg["gru_layers"],
        encoder_bidirectional=cfg["bidirectional"], encoder_fc_hidden_sizes=cfg["fc_hidden"],
        encoder_learnable_inital_state=cfg["learnable_h0"], encoder_fc_activation_function=cfg["fc_activation"])
    brain = bfe.bfe_w_preprocessing_from_config(args, None, name)
    return w2v.W2VBrainEncoderModel(w2v.W2VBrainEncoderModelArgs(w2v_do_stable_layer_norm=False), brain, name, None,
                                    True)


def run(act, modules, res):
    tfw, bfe, w2v, base_args = modules
    cfg = tiny_act_config(act)
    torch.manual_seed(0)
    model = build_reference_model(cfg, tfw, bfe, w2v, base_args)
    sd = deterministic_state([(n, p.shape) for n, p in model.named_parameters()], seed=cfg["seed"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(("gaussian_smoother.weight", "inv_freq")) for k in missing), missing
    model.train()   # deterministic: every dropout and layerdrop is 0
    from src.datasets.batch_types import B2tSampleBatch
    x, day, in_lens, tgt, tgt_lens = make_batch(cfg)
    batch = B2tSampleBatch(x, tgt)
    batch.day_idxs = day
    batch.input_lens = in_lens
    batch.target_lens = tgt_lens
    out = model.forward(batch)
    out.loss.backward()
    if "x" not in res:
        res.update({"x": x.numpy(), "day_idxs": day.numpy(), "input_lens": in_lens.numpy(), "target": tgt.numpy(),
                    "target_lens": tgt_lens.numpy(), "names": np.array(NAMES),
                    "param_names": np.array([n for n, _ in model.named_parameters()])})
    else:
        assert np.array_equal(res["x"], x.numpy())
    res[f"{act}/loss"] = np.array(out.loss.item(), dtype=np.float64)
    res[f"{act}/logits"] = out.logits.detach().numpy()
    for n, p in model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        res[f"{act}/gnorm/{n}"] = np.array(g.double().norm().item())
        if ".fc." in n:
            res[f"{act}/grad/{n}"] = g.numpy().copy()
    print(f"{act}: loss={out.loss.item():.6f}", flush=True)


if __name__ == "__main__":
    mods = mg._import_reference()
    torch.set_num_threads(8)
    res: dict = {}
    for a in NAMES:
        run(a, mods, res)
    path = os.path.join(mg.OUT, "tiny_act.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB")

"""The model's shape and its host-side constants: VAEConfig, the positional table, the reference's parameter list and its Xavier
initialiser. numpy only: importable without torch or the kernel library."""
import math
from collections import OrderedDict

import numpy as np


class VAEConfig:
    """Shape of the model: the union of ModelConfig/EncoderConfig/DecoderConfig/TransformerConfig
    (model.py:22-54, transformer.py:8-21) flattened, plus which ends are attached:
    kind='token' (Embedding in, softmax-CE out: the reference's executed path) or
    kind='pianoroll' (multi-hot frame x table in, sigmoid + BinaryCrossEntropy out)."""

    def __init__(self, kind, in_dim, out_dim, num_classes, latent_dim, e_model, e_layers, e_heads, d_model, d_layers,
                 d_heads, e_dropout=0.0, d_dropout=0.0, d_causal=False):
        assert kind in ("token", "pianoroll")
        assert e_model % e_heads == 0 and d_model % d_heads == 0  # transformer.py:134,167
        self.kind = kind
        self.in_dim, self.out_dim = in_dim, out_dim
        self.num_classes, self.latent_dim = num_classes, latent_dim
        self.e_model, self.e_layers, self.e_heads = e_model, e_layers, e_heads
        self.d_model, self.d_layers, self.d_heads = d_model, d_layers, d_heads
        self.e_dropout, self.d_dropout = float(e_dropout), float(d_dropout)
        # d_causal: the decoder's self-attention is causal with a softmax over the keys (mst_attn_causal_fwd/bwd), the model
        # DecodePlan(attention="key") samples from. Off: the reference's non-causal query-axis softmax (transformer.py:174,100).
        self.d_causal = bool(d_causal)

    def as_dict(self):
        return dict(self.__dict__)


def positional_table(model_size, max_len):
    """transformer.py:204-211: exponent 2*i/D for every column, sin on even / cos on odd columns,
    float64 then cast (host-side constant, built once)."""
    pos = np.arange(max_len).reshape((-1, 1)) / np.power(10000, (2.0 / model_size) * np.arange(model_size).reshape((1, -1)))
    pos[:, 0::2] = np.sin(pos[:, 0::2])
    pos[:, 1::2] = np.cos(pos[:, 1::2])
    return pos.astype(np.float32)


def logical_param_shapes(cfg):
    """name -> shape in the reference's construction order (model.py:57-71,206-227;
    transformer.py:24-46,49-68,129-149,162-182): 58 tensors at e_layers=2, d_layers=1."""
    s = OrderedDict()
    De, Dd, Z, C = cfg.e_model, cfg.d_model, cfg.latent_dim, cfg.num_classes

    def layer(prefix, D, last_ln):
        for w in ("W_k", "W_q", "W_v", "W_proj"):
            s[f"{prefix}.att.{w}.weight"] = (D, D)
            s[f"{prefix}.att.{w}.bias"] = (D,)
        s[f"{prefix}.ln1.gamma"] = (D,)
        s[f"{prefix}.ln1.beta"] = (D,)
        s[f"{prefix}.ff1.weight"] = (4 * D, D)
        s[f"{prefix}.ff1.bias"] = (4 * D,)
        s[f"{prefix}.ff2.weight"] = (D, 4 * D)
        s[f"{prefix}.ff2.bias"] = (D,)
        s[f"{prefix}.{last_ln}.gamma"] = (D,)
        s[f"{prefix}.{last_ln}.beta"] = (D,)

    s["encoder.class2hid.weight"] = (C, De)
    s["encoder.embedding.weight"] = (cfg.in_dim, De)
    for i in range(cfg.e_layers):
        layer(f"encoder.layer{i}", De, "ln2")
    s["encoder.latent_proj.weight"] = (2 * Z, De)
    s["encoder.latent_proj.bias"] = (2 * Z,)
    s["decoder.latent2hid.weight"] = (Dd, Z)
    s["decoder.latent2hid.bias"] = (Dd,)
    s["decoder.class2hid.weight"] = (C, Dd)
    s["decoder.embedding.weight"] = (cfg.out_dim, Dd)
    for i in range(cfg.d_layers):
        layer(f"decoder.layer{i}", Dd, "ln3")
    s["decoder.output_layer.weight"] = (cfg.out_dim, Dd)
    s["decoder.output_layer.bias"] = (cfg.out_dim,)
    return s


def xavier_init(cfg, rng):
    """trainer.py:103-105 model.initialize(mx.init.Xavier()): uniform, factor 'avg', magnitude 3 for
    every '*weight' (Embedding tables included); biases / beta 0; gamma 1."""
    out = OrderedDict()
    for name, shape in logical_param_shapes(cfg).items():
        if name.endswith("weight"):
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            scale = math.sqrt(3.0 / ((fan_in + fan_out) / 2.0))
            out[name] = rng.uniform(-scale, scale, size=shape).astype(np.float32)
        elif name.endswith("gamma"):
            out[name] = np.ones(shape, np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out

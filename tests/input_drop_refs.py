"""References for decoder-input dropout (include/mst_hip.h: mst_step_begin_args.in_*), no GPU and no library: the masked row copy, the
token embedding forward / backward with a keep mask in fp64, and oracle.vae_oracle.decode_train restated with the input embedding
multiplied by the mask — installed on the imported oracle module for the duration of a comparison (masked_decoder), the oracle's files
stay as they are."""
import contextlib

import numpy as np
import torch

IN_SITE = 0x7FFF0001  # ops.IN_SITE, restated


def masked_rows(src, keep, row_bytes, dst):
    """dst [n, ld_dst] after the launch: bytes [0, row_bytes) of row r are src's where keep[r], zero where not; the rest of the row is
    what dst held. src [n, ld_src], dst uint8 arrays, keep [n] of 0 / 1"""
    out = np.array(dst, copy=True)
    out[:, :row_bytes] = np.where(np.asarray(keep).astype(bool)[:, None], src[:, :row_bytes], 0)
    return out


def embed_fwd(tokens, table, pos, alpha, s_off, keep=None, classes=None, cls_table=None):
    """fp64 [B, T, D]: alpha * ((keep ? table[tok] : 0) + cls[c_b]) + pos[s_off + t]. alpha is the launch's fp32 scalar. Every product
    of two fp32 values is exact in fp64, so rounding this once to fp32 is what a fused multiply-add gives."""
    tokens = np.asarray(tokens)
    B, T = tokens.shape
    e = np.asarray(table, np.float64)[tokens]
    if keep is not None:
        e = e * np.asarray(keep, np.float64).reshape(B, T, 1)
    if cls_table is not None:
        e = e + np.asarray(cls_table, np.float64)[np.asarray(classes)][:, None, :]
    return float(np.float32(alpha)) * e + np.asarray(pos, np.float64)[s_off: s_off + T][None]


def embed_bwd(tokens, dX, alpha, V, keep=None, classes=None, n_classes=0):
    """fp64 (dtable [V, D], dcls [n_classes, D] or None) of the forward above: row (b, t) of alpha * dX goes to table row tok[b, t] unless
    it was dropped, and to class row c_b either way. dX [B, T, D]: the rows s_off.. of the launch's gradient"""
    tokens = np.asarray(tokens)
    B, T = tokens.shape
    g = float(np.float32(alpha)) * np.asarray(dX, np.float64)
    gk = g if keep is None else g * np.asarray(keep, np.float64).reshape(B, T, 1)
    dtable = np.zeros((V, g.shape[-1]))
    np.add.at(dtable, tokens.reshape(-1), gk.reshape(B * T, -1))
    dcls = None
    if n_classes:
        dcls = np.zeros((n_classes, g.shape[-1]))
        np.add.at(dcls, np.asarray(classes), g.sum(1))
    return dtable, dcls


_KEEP = [None]  # the mask masked_decoder installed: [B, T] of 0 / 1


def decode_train(P, cfg, x, seq_lens, z, classes, masks):
    """oracle.vae_oracle.decode_train (Decoder.forward_train, model.py:237-257) with ONE change: the input embedding of position k is
    multiplied by keep[b, k] — a dropped position contributes a zero embedding, so its decoder input row is sqrt(D) * 0 + pos[k + 1]"""
    from oracle import vae_oracle as O
    B, T = x.shape[0], x.shape[1]
    dt = z.dtype
    Dd = cfg.d_model
    tok = O.input_embedding(cfg, P["decoder.embedding.weight"], x)
    tok = tok * torch.as_tensor(np.asarray(_KEEP[0]).reshape(B, T, 1)).to(dt)  # <- the change
    init = O.dense(z, P["decoder.latent2hid.weight"], P["decoder.latent2hid.bias"]) + P["decoder.class2hid.weight"][classes.long()]
    h = torch.cat([init[:, None, :], tok], dim=1)
    valid = (torch.arange(T + 1)[None, :] < (seq_lens.long() + 1)[:, None]).to(dt)
    pos = torch.from_numpy(O.positional_encodings(Dd, T + 1)).to(dt)
    h = torch.sqrt(torch.tensor(float(Dd), dtype=dt)) * h + pos
    for i in range(cfg.d_layers):
        h = O.decoder_layer(P, f"decoder.layer{i}", h, valid, cfg.d_heads, masks)
    h = h[:, 1:, :]
    return O.dense(h, P["decoder.output_layer.weight"], P["decoder.output_layer.bias"])


@contextlib.contextmanager
def masked_decoder(keep):
    """oracle.vae_oracle.decode_train replaced by the masked restatement for the duration of the block (keep: [B, T] or [B * T], the
    device's in_keep of that step), the original restored afterwards"""
    from oracle import vae_oracle as O
    original, before = O.decode_train, _KEEP[0]
    O.decode_train, _KEEP[0] = decode_train, np.asarray(keep)
    try:
        yield
    finally:
        O.decode_train, _KEEP[0] = original, before

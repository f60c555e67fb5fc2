"""The reference of VH_FLAG_SUB_LN (TEST INFRASTRUCTURE), on top of swiglu_ref and vit_ref, which it does not change: the blob with
subln.width, subln.weight and subln.bias at its end, the gate with the inner LayerNorm over the true width n (float64, or with the
device's roundings: g and u as fc1 stores them, h rounded once), a forward, and the seeded EVA-02 state dicts of tests/golden/eva02.
The fixtures store no weights (fixture b's are 6 MB): they are regenerated from numpy.random.default_rng(seed) -- PCG64 and
standard_normal, whose streams numpy keeps stable by policy (NEP 19); a change of them fails test_subln's 1e-14 comparison loudly."""
import glob
import os

import numpy as np

import swiglu_ref as W
import vh_synth as S
import vit_ref as R

FLAG_SUB_LN = 1 << 29
SMALL = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=384, layers=2, classes=40)
# name: (cfg, true gated width n, fc_norm mean-pool head, weight seed, image seed, batch); a takes the plain layer loop, b the folded one
# c is a with n = 346 = 43 * 8 + 2: the width ends inside a 16-byte chunk, as EVA-02-L's 2730 does
FIXTURES = {"a": (SMALL, 344, False, 301, 302, 3), "b": (dict(SMALL, dim=256, heads=4, mlp_dim=768), 688, True, 303, 304, 3),
            "c": (SMALL, 346, False, 305, 306, 3)}


def tensor_table(cfg, flags):
    sub = [("subln.width", (1,)), ("subln.weight", (cfg["layers"], cfg["mlp_dim"])), ("subln.bias", (cfg["layers"], cfg["mlp_dim"]))]
    return [(n, s) for n, s, *_ in W.tensor_table(cfg, flags & ~FLAG_SUB_LN)] + (sub if flags & FLAG_SUB_LN else [])


def blob_bytes(cfg, flags):
    return 64 + 4 * sum(int(np.prod(s)) for _, s in tensor_table(cfg, flags))


def unpack_blob(cfg, blob, flags):
    assert blob.size == blob_bytes(cfg, flags)
    sizes = [int(np.prod(s)) for _, s in tensor_table(cfg, flags)]
    parts = np.split(blob[64:].view(np.float32), np.cumsum(sizes)[:-1])
    return {n: p.reshape(s) for (n, s), p in zip(tensor_table(cfg, flags), parts)}


def gate_ln(M, n, w, b, eps, q16=None):
    """z [rows, 2 M] -> h [rows, M] = LN_n(silu(g) * u) * w + b, zero from column n on.  q16 rounds z before and h after, nothing else."""
    def act(z):
        z = q16(z).astype(z.dtype) if q16 is not None else z
        h = np.zeros_like(z[:, :M])
        h[:, :n] = R.layernorm(W.silu(z[:, :n]) * z[:, M:M + n], w[:n], b[:n], eps)
        return q16(h).astype(z.dtype) if q16 is not None else h
    return act


def forward(cfg, t, images, flags, eps, dtype=np.float64, q16=None):
    """Logits of a ROPE | SWIGLU | SUB_LN model with a class token from its blob tensors t (vit_ref's layer, this gate)."""
    t = {k: np.asarray(v).astype(dtype) for k, v in t.items()}
    D, H, M, n = cfg["dim"], cfg["heads"], cfg["mlp_dim"], int(t["subln.width"][0])
    x = R.assemble(R.patch_embed(cfg, t, np.asarray(images, dtype)), t["cls"], t["pos"])
    batch, T, _ = x.shape
    x = x.reshape(batch * T, D)
    for l in range(cfg["layers"]):
        act = gate_ln(M, n, t["subln.weight"][l], t["subln.bias"][l], eps, q16)
        x = R.layer(x, lambda name: t[f"l{l}.{name}"], act, batch, T, H, D // H, eps, None, (t["rope.cos"], t["rope.sin"], 1))
    hin = R.head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], eps, 1, R.pool_of(flags))
    return hin @ t["head.weight"].T + t["head.bias"]


def fixture_state_dict(name):
    """A seeded EVA-02 state dict under timm's key names (separate q / k / v projections, q and v bias, no k bias, mlp.norm)."""
    cfg, n, mean, seed, *_ = FIXTURES[name]
    D, NP, rng = cfg["dim"], (cfg["image_size"] // cfg["patch_size"]) ** 2, np.random.default_rng(seed)
    lin = lambda o, i: (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    vec = lambda k, s=0.05, m=0.0: (m + s * rng.standard_normal(k)).astype(np.float32)
    sd = {"patch_embed.proj.weight": lin(D, cfg["channels"] * cfg["patch_size"] ** 2).reshape(D, cfg["channels"], cfg["patch_size"], cfg["patch_size"]),
          "patch_embed.proj.bias": vec(D), "cls_token": vec(D, 0.5).reshape(1, 1, D), "pos_embed": vec((NP + 1) * D, 0.5).reshape(1, NP + 1, D),
          ("fc_norm" if mean else "norm") + ".weight": vec(D, 0.1, 1.0), ("fc_norm" if mean else "norm") + ".bias": vec(D),
          "head.weight": lin(cfg["classes"], D), "head.bias": vec(cfg["classes"])}
    for l in range(cfg["layers"]):
        b = f"blocks.{l}."
        for nm, k in (("norm1", D), ("norm2", D), ("mlp.norm", n)):
            sd[b + nm + ".weight"], sd[b + nm + ".bias"] = vec(k, 0.1, 1.0), vec(k)
        for nm, (o, i) in (("attn.q_proj", (D, D)), ("attn.k_proj", (D, D)), ("attn.v_proj", (D, D))):
            sd[b + nm + ".weight"] = lin(o, i)
        sd[b + "attn.q_bias"], sd[b + "attn.v_bias"] = vec(D), vec(D)
        for nm, (o, i) in (("attn.proj", (D, D)), ("mlp.fc1_g", (n, D)), ("mlp.fc1_x", (n, D)), ("mlp.fc2", (D, n))):
            sd[b + nm + ".weight"], sd[b + nm + ".bias"] = lin(o, i), vec(o)
        for nm in ("attn.proj", "mlp.fc2"):    # residual updates a third of the stream's size, as LayerScale or a depth-scaled init leaves them
            sd[b + nm + ".weight"] *= np.float32(0.3)
    return sd


def width_at(cfg, blob):
    """Byte offset of the subln.width word: in front of the two [layers][M] tensors that end the blob."""
    return blob.size - 4 * (1 + 2 * cfg["layers"] * cfg["mlp_dim"])


def fixture(name, eps=1e-6):
    """(npz, cfg, flags, the blob the EVA-02 converter makes of the seeded state dict, its tensors)"""
    import vithip
    path, = glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eva02", name + "_s*.npz"))
    cfg = FIXTURES[name][0]
    blob = vithip.blob_from_eva02_state_dict(fixture_state_dict(name), cfg, eps)
    flags = vithip.blob_flags_of(blob)
    return np.load(path), cfg, flags, blob, unpack_blob(cfg, blob, flags)


def fixture_images(name):
    cfg, _, _, _, iseed, batch = FIXTURES[name]
    return S.make_images(cfg, iseed, batch)

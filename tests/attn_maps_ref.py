"""Reference of the attention maps (include/vithip.h, "Attention maps"; TEST INFRASTRUCTURE): the float64 softmax rows of an image's
first Q queries, a numpy emulation of the read-out kernel, and the float64 probabilities of one layer of the reference model.  No GPU.

Everything is in the exp2 domain, as the kernels are: q arrives scaled by head_dim^-1/2 * log2(e), p[t] = 2^(s[t] - max s) / sum.
Shapes: q|k|v row-major [batch * T][3 * heads * hd]; probabilities [batch][heads][Q][T]."""
import math

import numpy as np

import attn_exact as AX
import vit_ref as RR
import vithip

LOG2E = 1.4426950408889634
NP_DTYPE = {vithip.ELEM_F32: np.float32, vithip.ELEM_F16: np.uint16, vithip.ELEM_BF16: np.uint16}
ELEM_DTYPE = {vithip.ELEM_F16: vithip.DTYPE_FP16, vithip.ELEM_BF16: vithip.DTYPE_BF16}


def scores(qkv, batch, tokens, heads, hd, Q):
    """float64 log2-domain scores [batch][heads][Q][tokens] of the first Q rows of every image."""
    x = np.asarray(qkv, dtype=np.float64).reshape(batch, tokens, 3, heads, hd)
    return np.einsum("bqhd,bthd->bhqt", x[:, :Q, 0], x[:, :, 1])


def probs64(qkv, batch, tokens, heads, hd, Q):
    """The float64 reference: softmax rows of the first Q queries."""
    s = scores(qkv, batch, tokens, heads, hd, Q)
    e = np.exp2(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def exact32(qkv, batch, tokens, heads, hd, Q):
    """What the kernel must write BIT FOR BIT when every score is an exact integer and the row sum is exact in fp32 (the designs of
    attn_exact at tokens <= 1024, `uniform` at any size): np.float32(e) / np.float32(l), one IEEE division."""
    s = scores(qkv, batch, tokens, heads, hd, Q)
    assert np.array_equal(s, np.round(s)), "the scores are not integers"
    e = np.exp2(s - s.max(-1, keepdims=True))
    l = e.sum(-1, keepdims=True)
    # (a power of two converts to fp32 exactly, or underflows to 0 below 2^-149, which is what exp2 gives as well)
    # l: exact in fp32, or 1 + a tail below half an ulp of 1 (permutation), which every fp32 summation order rounds to 1
    assert np.array_equal(l.astype(np.float32).astype(np.float64), l) or (np.abs(l - 1.0) < 2.0 ** -25).all(), "the row sum is not exact in fp32"
    with np.errstate(under="ignore"):
        return (e.astype(np.float32) / l.astype(np.float32)).astype(np.float32)


def to_elem(a32, elem):
    """fp32 values -> the read-out's element type: fp32 as it is, 16-bit = RNE bits through vithip.to16."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    return a32 if elem == vithip.ELEM_F32 else vithip.to16(a32, ELEM_DTYPE[elem])


def readout(store, lead, elem, keys):
    """The read-out kernel in numpy.  store fp32 [B][H][Q][T] -> (probs [B][H][Q][K], head_mean [B][Q][K]) in `elem`: the key slice,
    the serial fp32 chain (((0 + p[0]) + p[1]) + ...) * float32(1 / H) of the unrounded values, RNE to 16 bit."""
    store = np.ascontiguousarray(store, dtype=np.float32)
    k0 = lead if keys == vithip.ATTN_KEYS_PATCH else 0
    p = store[..., k0:]
    acc = np.zeros(p[:, 0].shape, dtype=np.float32)
    for h in range(p.shape[1]):
        acc = (acc + p[:, h]).astype(np.float32)
    mean = (acc * np.float32(1.0 / p.shape[1])).astype(np.float32)
    return to_elem(p, elem), to_elem(mean, elem)


def widen(a, elem):
    """A read-out array (uint16 bits for the 16-bit element types) -> float32 values."""
    return np.asarray(a, dtype=np.float32) if elem == vithip.ELEM_F32 else vithip.from16(a, ELEM_DTYPE[elem])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(bits(a), bits(b))


def layer_probs64(cfg, blob, hidden, k, batch, Q, flags=0, ln_eps=1e-6):
    """float64 probabilities [batch][heads][Q][T] of encoder layer k (1-based) from vit_ref.forward(..., all_hidden=True)'s list:
    LN1 of hidden[k - 1], the q and k projections, the scale, softmax (natural exponent, as the model is written)."""
    t = {n: v.astype(np.float64) for n, v in RR.unpack_blob(cfg, blob, flags).items()}
    D, H = cfg["dim"], cfg["heads"]
    hd = D // H
    x = np.asarray(hidden[k - 1], dtype=np.float64)
    T = x.shape[0] // batch
    p = lambda n: t[f"l{k - 1}.{n}"]
    y = RR.layernorm(x, p("ln1.weight"), p("ln1.bias"), ln_eps)
    q = (y @ p("q.weight").T + p("q.bias")).reshape(batch, T, H, hd)[:, :Q]
    kk = (y @ p("k.weight").T + p("k.bias")).reshape(batch, T, H, hd)
    s = np.einsum("bqhd,bthd->bhqt", q, kk) / math.sqrt(hd)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def self_test():
    """The reference on attn_exact's designs: uniform gives 1 / T correctly rounded, permutation 1 at pi and less than 2^-24 elsewhere,
    graded rows sum to 1."""
    B, T, H, hd, Q = 2, 37, 3, 64, 5
    u = AX.make_case("uniform", B, T, H, hd, seed=3)
    assert (exact32(u.qkv, B, T, H, hd, Q) == np.float32(1) / np.float32(T)).all()
    assert np.allclose(probs64(u.qkv, B, T, H, hd, Q), 1.0 / T, rtol=1e-15)
    pm = AX.make_case("permutation", B, T, H, hd, seed=3)
    p = exact32(pm.qkv, B, T, H, hd, Q)
    at = np.zeros(p.shape, dtype=bool)
    np.put_along_axis(at, pm.pi[:, :, :Q, None], True, axis=-1)
    assert (p[at] == 1.0).all() and (p[~at] < 2.0 ** -24).all()
    g = AX.make_case("graded", B, T, H, hd, seed=3)
    assert np.abs(probs64(g.qkv, B, T, H, hd, Q).sum(-1) - 1.0).max() < 1e-14
    assert np.abs(exact32(g.qkv, B, T, H, hd, Q).astype(np.float64).sum(-1) - 1.0).max() <= (T + 8) * 2.0 ** -24
    return True

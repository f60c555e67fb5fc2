#!/usr/bin/env python3
"""Generate tests/golden/ref_digests.json -- the SHA-256 of the reference's seeded blob, make_blob(cfg, seed, flags), for every legal
flag word the model-flag tests enumerate (tests/test_pool.py's grid, the LEGAL lists of tests/test_siglip.py and tests/test_rope.py),
on two shapes (vit_micro and one of head dim 80) with two seeds.  tests/test_ref_digests.py holds tests/vit_ref.py to the file, so
that a change of the blob's order, of a tensor id or of a header bit shows as a changed digest.

The committed file was written at commit 60c72d2, the last one at which the reference was three modules (vit_ref, siglip_ref on top
of it, rope_ref on top of both), from the topmost of them:  python tests/golden/make_ref_digests.py --module rope_ref
Since then tests/vit_ref.py is the one module and the default.  Needs numpy only.  Re-run:  python tests/golden/make_ref_digests.py
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vh_synth as S

# the flag values of include/vithip.h, stated here once more: the file must not move when a module's constants do
PRE, QUICK, NO_CLS, MAP, TANH, ROPE = 16, 32, 1 << 15, 1 << 19, 1 << 21, 1 << 23
CLS, AVG_NORM, AVG_FCNORM, CLS_AVG = range(4)


def REG(n):
    return n << 9


def POOL(m):
    return m << 16


SHAPES = {"vit_micro": S.CONFIGS["vit_micro"],
          "hd80": dict(image_size=48, patch_size=16, channels=3, dim=320, heads=4, mlp_dim=384, layers=2, classes=8)}
SEEDS = (5, 9)
POOL_GRID = [0, PRE, QUICK, PRE | QUICK, REG(1), REG(4), PRE | QUICK | REG(1)] \
    + [nc | POOL(m) | REG(n) for nc in (0, NO_CLS) for m in range(4) for n in (0, 4) if not nc or m in (AVG_NORM, AVG_FCNORM)] \
    + [NO_CLS | POOL(AVG_FCNORM) | REG(4) | PRE | QUICK]
SIGLIP_LEGAL = [TANH, TANH | PRE, TANH | REG(4), TANH | POOL(CLS_AVG), TANH | NO_CLS | POOL(AVG_NORM), TANH | NO_CLS | POOL(AVG_FCNORM) | REG(2),
                MAP | NO_CLS, MAP | NO_CLS | TANH, MAP | NO_CLS | QUICK, MAP | NO_CLS | PRE, MAP | NO_CLS | TANH | PRE]
ROPE_LEGAL = [ROPE, ROPE | REG(4), ROPE | PRE | QUICK, ROPE | TANH, ROPE | POOL(CLS_AVG), ROPE | NO_CLS | POOL(AVG_NORM),
              ROPE | NO_CLS | REG(2) | POOL(AVG_FCNORM), ROPE | MAP | NO_CLS | TANH]
FLAG_WORDS = sorted(set(POOL_GRID + SIGLIP_LEGAL + ROPE_LEGAL + [f & ~ROPE for f in ROPE_LEGAL]))      # (each ROPE word also without the bit)


def digests(ref):
    return {shape: {str(seed): {str(f): hashlib.sha256(ref.make_blob(cfg, seed, f).tobytes()).hexdigest() for f in FLAG_WORDS}
                    for seed in SEEDS} for shape, cfg in SHAPES.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--module", default="vit_ref")
    ap.add_argument("--out", default=os.path.join(HERE, "ref_digests.json"))
    a = ap.parse_args()
    doc = {"function": "sha256(make_blob(cfg, seed, flags).tobytes())", "shapes": SHAPES, "make_blob": digests(importlib.import_module(a.module))}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(FLAG_WORDS), "flag words x", len(SHAPES), "shapes x", len(SEEDS), "seeds ->", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()

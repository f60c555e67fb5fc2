"""The reference's seeded blobs against their recorded digests, and the three statements of the blob's order against each other: the
library's (vh_weight_blob_bytes), the product Python's (vithip.blob_tensor_table) and the reference's (vit_ref.tensor_table).
tests/golden/ref_digests.json was written by tests/golden/make_ref_digests.py before the model flags' reference modules were merged
into tests/vit_ref.py: a change of the blob's order, of a seeded tensor's id or of a header bit shows here.  No GPU needed."""
import json
import os

import numpy as np
import pytest

import test_pool
import test_rope
import test_siglip
import vit_ref as R
from vh_testlib import blob_digest, lib_blob_bytes

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
LEGAL = sorted(set(test_pool.LEGAL + test_siglip.LEGAL + test_rope.LEGAL))
VIT_B = dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=768)


def test_make_blob_has_the_recorded_digests():
    path = os.path.join(HERE, "golden", "ref_digests.json")
    assert os.path.getsize(path) < 20 * 1024
    with open(path) as f:
        doc = json.load(f)
    assert set(doc["shapes"]) == {"vit_micro", "hd80"} and doc["shapes"]["vit_micro"] == test_pool.MICRO and doc["shapes"]["hd80"] == test_rope.HD80
    n = 0
    for shape, by_seed in doc["make_blob"].items():
        assert len(by_seed) == 2
        for seed, by_flags in by_seed.items():
            assert set(LEGAL) <= {int(f) for f in by_flags}                     # every LEGAL list of the model-flag tests is recorded
            for flags, want in by_flags.items():
                assert R.legal(doc["shapes"][shape], int(flags)), flags
                assert blob_digest(R.make_blob(doc["shapes"][shape], int(seed), int(flags))) == want, (shape, seed, flags)
                n += 1
    assert n >= 4 * len(LEGAL)


def test_blob_tensor_table_is_the_references_and_sums_to_the_librarys_bytes():
    for cfg in (test_pool.MICRO, test_rope.HD80, VIT_B):
        for flags in LEGAL:
            assert vithip.blob_tensor_table(cfg, flags) == [(name, tuple(shape)) for name, shape, *_ in R.tensor_table(cfg, flags)], flags
            n = sum(int(np.prod(shape)) for _, shape in vithip.blob_tensor_table(cfg, flags))
            assert 64 + 4 * n == lib_blob_bytes(cfg, flags) > 0, flags

"""The small helpers the test modules share (TEST INFRASTRUCTURE).  A module whose own variant differs keeps it.

A GPU module that uses `dev` imports the fixture by name with it, `from vh_testlib import dev, _release_buffers`: pytest runs an
autouse fixture that stands in the module's namespace, and the buffers of a test are freed when it ends."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import vithip


def rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def last_error():
    return vithip.lib().vh_last_error(None).decode()


def vit_cfg(image, patch, dim, heads, mlp, layers, classes, channels=3):
    return dict(image_size=image, patch_size=patch, channels=channels, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=classes)


def lib_blob_bytes(cfg, flags=0, dtype=vithip.DTYPE_BF16, max_batch=1, ln_eps=1e-6):
    c = vithip.make_config(cfg, dtype, max_batch, ln_eps, flags)
    return vithip.lib().vh_weight_blob_bytes(C.byref(c))


def blob_digest(blob):
    return hashlib.sha256(np.ascontiguousarray(blob, dtype=np.uint8).tobytes()).hexdigest()


def recorded_blob_digest(shape, seed, flags):
    """The SHA-256 of the reference's make_blob(SHAPES[shape], seed, flags) as tests/golden/ref_digests.json records it
    (tests/golden/make_ref_digests.py; shapes "vit_micro" and "hd80", seeds 5 and 9)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")) as f:
        return json.load(f)["make_blob"][shape][str(seed)][str(flags)]


_KEEP = []


def dev(a):
    """Upload and keep the allocation alive until the test ends (a temporary DeviceBuffer would be freed by its destructor before
    the kernel that reads it runs)."""
    b =vithip.DeviceBuffer.from_numpy(a)
    _KEEP.append(b)
    return b


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    for b in _KEEP:
        b.free()
    _KEEP.clear()

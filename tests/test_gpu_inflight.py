"""Two forwards in flight (include/vithip.h, vh_forward_device_async): consecutive steps of one call and consecutive submits of an
image ring alternate between two compute streams and two sets of activation buffers.  Nothing inside a forward changes, so
every comparison here is equality of bits with the synchronous, one-at-a-time forward of the same images.

Overlap needs a forward that outlasts the host's enqueue of the next one (about 1 ms of launches): those cases run ViT-B/16 at
batch 64 (about 3 ms per forward).  The plumbing cases run SMALL at batch 40: the folded, split-residual path (row statistics,
partial sums and attention tickets in use), 1 480 rows = 5.8 row tiles, bf16 and e4m3 operands.

What a test can see of the ORDER of the two streams: the library's streams are non-blocking, so a DeviceBuffer copy (a plain
hipMemcpy) is ordered behind nothing by itself.  The ordering points a caller has are the ones the header names: the event
behind the call (last_kernel_ms waits for it and for nothing else), a following call on the context (the feature read-out is
enqueued on the context's stream) and synchronize().  The logits of every step of one call are equal, so it is the read-outs
of the last step's residual rows -- which live in the second buffer set after an even number of steps -- that would show a
context's stream that did not wait for the second one."""
import numpy as np
import pytest

import vh_synth as S
import vithip
from vh_testlib import same_bits, vit_cfg

pytestmark = pytest.mark.gpu

BF16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP8
SMALL = vit_cfg(96, 16, 256, 4, 512, 2, 8)
SMALL_B, BASE_B = 40, 64
MODELS = {"base_bf16": (S.CONFIGS["vit_base"], BF16, BASE_B), "small_bf16": (SMALL, BF16, SMALL_B), "small_fp8": (SMALL, FP8, SMALL_B)}


def pixels(cfg):
    return cfg["image_size"] ** 2 * cfg["channels"]


class Model:
    """A context with seeded weights, seeded images resident in HBM and the logits of ONE synchronous forward of them."""

    def __init__(self, name, image_seed=1):
        self.cfg, self.dtype, self.B = MODELS[name]
        self.ctx = vithip.VitContext(self.cfg, dtype=self.dtype, max_batch=self.B)
        self.ctx.init_weights_seeded(3)
        assert self.ctx.ln_fold()                       # the folded path: statistics, partial sums, the split residual
        self.din = vithip.DeviceBuffer(self.B * pixels(self.cfg) * 4)
        self.dout = vithip.DeviceBuffer(self.B * self.cfg["classes"] * 4)
        self.ctx.fill_input_seeded(image_seed, self.B, self.din.ptr)
        self.ctx.forward_device(self.din.ptr, self.B, self.dout.ptr)
        self.want = self.logits()
        assert np.isfinite(self.want).all()

    def logits(self):
        return self.dout.to_numpy(np.float32, (self.B, self.cfg["classes"]))

    def poison(self):
        nan = vithip.DeviceBuffer.from_numpy(np.full((self.B, self.cfg["classes"]), np.nan, dtype=np.float32))
        self.dout.free()
        self.dout = nan

    def steps(self, k):
        self.ctx.forward_device_async(self.din.ptr, self.B, self.dout.ptr, steps=k)

    def close(self):
        self.ctx.close()
        self.din.free()
        self.dout.free()


@pytest.fixture(scope="module", params=list(MODELS))
def model(request):
    m = Model(request.param)
    yield m
    m.close()


@pytest.fixture
def small():
    m = Model("small_bf16")
    yield m
    m.close()


@pytest.mark.parametrize("steps", [7, 8])
def test_steps_of_one_call_run_two_at_a_time_and_leave_the_logits_of_one_forward(model, steps):
    """Odd and even step counts: the last step runs on the context's stream / on the second one.  The event behind the call
    (all that last_kernel_ms waits for) already covers every step of both streams; so does synchronize()."""
    m = model
    assert m.ctx.get_inflight() == 2
    m.poison()
    m.steps(steps)
    assert m.ctx.get_inflight() == 2
    assert m.ctx.last_kernel_ms() > 0.0         # waits for the event behind the call, not for the streams
    behind_event = m.logits()
    m.ctx.synchronize()
    assert same_bits(behind_event, m.want)
    assert same_bits(m.logits(), m.want)


def test_ring_submits_alternate_between_the_sets_and_collect_in_order_with_their_own_logits():
    """3 slots, 7 submits of 7 different image sets, ViT-B/16 at batch 64 so that consecutive forwards really overlap.  A buffer
    left shared between the sets (tickets, partial sums, statistics) would mix the rows of two image sets here."""
    cfg, dtype, B = MODELS["base_bf16"]
    m = Model("base_bf16")
    shape = (B, cfg["image_size"], cfg["image_size"], cfg["channels"])
    sets, wants = [], []
    for seed in range(11, 18):
        m.ctx.fill_input_seeded(seed, B, m.din.ptr)
        m.ctx.forward_device(m.din.ptr, B, m.dout.ptr)
        sets.append(m.din.to_numpy(np.float32, shape))
        wants.append(m.logits())
    assert not same_bits(wants[0], wants[1])
    m.ctx.ring_create(3, B)
    assert m.ctx.get_inflight() == 2
    got = []
    for images in sets:
        if m.ctx.ring_free_slots() == 0:
            got.append(m.ctx.ring_collect())
        m.ctx.ring_submit(images)
    while m.ctx.ring_free_slots() < 3:
        got.append(m.ctx.ring_collect())
    m.close()
    assert len(got) == 7
    for i, (g, w) in enumerate(zip(got, wants)):
        assert same_bits(g, w), f"collect {i} is not the forward of submit {i}"


def read_outs(ctx, cfg, B):
    T, D = S.tokens(cfg), cfg["dim"]
    out = ctx.read_features(cls=True, patch=True, mean=True)
    out["residual"] = ctx.debug_read(0, B * T * D)
    out["head_input"] = ctx.debug_read(1, B * D)
    return out


@pytest.mark.parametrize("name", ["small_bf16", "small_fp8"])
def test_read_outs_of_the_last_forward_read_the_last_steps_buffer_set(name):
    """After 2 steps the last forward's rows live in the second set, after 3 in the first: features and debug taps equal those
    of a single forward either way.  The device form is enqueued right behind the call, with no synchronise in between: the
    context's stream has to be behind the second stream for it to read finished rows."""
    m = Model(name)
    cfg, B, D = m.cfg, m.B, m.cfg["dim"]
    want = read_outs(m.ctx, cfg, B)
    for steps in (2, 3):
        m.steps(steps)
        got = read_outs(m.ctx, cfg, B)
        for k in want:
            assert same_bits(got[k], want[k]), (steps, k)
    NP = S.tokens(cfg) - 1
    dcls, dpatch = vithip.DeviceBuffer(B * D * 4), vithip.DeviceBuffer(B * NP * D * 4)
    m.steps(2)
    m.ctx.read_features_device_async(vithip.Features(dcls.ptr, dpatch.ptr, None, vithip.ELEM_F32, vithip.FEAT_NORM))
    m.ctx.synchronize()
    assert same_bits(dcls.to_numpy(np.float32, (B, D)), want["cls"])
    assert same_bits(dpatch.to_numpy(np.float32, (B, NP, D)), want["patch"])
    m.close()


def test_the_last_set_follows_single_forwards_and_ring_submits(small):
    """Two image sets, so that the two buffer sets hold different rows: a single forward after a two-step call is read from the
    first set, and after ring submits of a then b (first set, second set) the read-outs are b's."""
    m = small
    cfg, B = m.cfg, m.B
    a = m.din.to_numpy(np.float32, (B, cfg["image_size"], cfg["image_size"], cfg["channels"]))
    b = S.make_images(cfg, 2, B)
    assert same_bits(m.ctx.forward(a), m.want)
    want_a = read_outs(m.ctx, cfg, B)
    logits_b = m.ctx.forward(b)
    want_b = read_outs(m.ctx, cfg, B)
    assert not same_bits(want_a["cls"], want_b["cls"])
    m.steps(2)                                   # both sets hold a's rows
    assert same_bits(m.ctx.forward(b), logits_b)  # the first set holds b's
    got = read_outs(m.ctx, cfg, B)
    for k in want_b:
        assert same_bits(got[k], want_b[k]), k
    m.ctx.ring_create(2, B)
    m.ctx.ring_submit(a)
    m.ctx.ring_submit(b)
    assert same_bits(m.ctx.ring_collect(), m.want) and same_bits(m.ctx.ring_collect(), logits_b)
    vithip.lib().vh_ring_destroy(m.ctx.h)
    got = read_outs(m.ctx, cfg, B)
    for k in want_b:
        assert same_bits(got[k], want_b[k]), k


FALLBACKS = {
    "stage_timing": lambda ctx: ctx.set_stage_timing("fc1_gemm"),
    "streams": lambda ctx: ctx.set_streams(2),
    "graph": lambda ctx: ctx.set_graph(True),
    "feature_layers": lambda ctx: ctx.set_feature_layers([1]),
}


@pytest.mark.parametrize("how", list(FALLBACKS))
def test_fallbacks_run_one_forward_at_a_time_with_unchanged_results(small, how):
    m = small
    assert m.ctx.get_inflight() == 2
    FALLBACKS[how](m.ctx)
    assert m.ctx.get_inflight() == 1
    m.poison()
    m.steps(6)
    m.ctx.synchronize()
    assert same_bits(m.logits(), m.want)
    if how == "stage_timing":
        assert m.ctx.get_stage_timing()[2] == 6 * m.cfg["layers"]
        m.ctx.set_stage_timing(None)
        assert m.ctx.get_inflight() == 2


def test_step_timing_runs_one_forward_at_a_time(small):
    m = small
    m.ctx.set_step_timing(True)
    assert m.ctx.get_inflight() == 1
    m.steps(4)
    m.ctx.synchronize()
    assert len(m.ctx.get_step_timing()) == 4 and same_bits(m.logits(), m.want)


def test_vh_inflight_1_in_the_environment_keeps_a_context_single_flight(monkeypatch):
    monkeypatch.setenv("VH_INFLIGHT", "1")
    m = Model("small_bf16")
    monkeypatch.delenv("VH_INFLIGHT")
    two = Model("small_bf16")
    assert m.ctx.get_inflight() == 1 and two.ctx.get_inflight() == 2   # read when the context is created
    for x in (m, two):
        x.poison()
        x.steps(6)
        x.ctx.synchronize()
    assert same_bits(m.logits(), two.logits()) and same_bits(m.logits(), m.want)
    m.close()
    two.close()


def test_rehearsal_group_members_run_their_steps_two_at_a_time():
    """Two members on device 0, each with its own context, streams and buffer sets: four forwards share the GPU."""
    blob = S.make_blob(SMALL, 5)
    g = vithip.VitGroup(SMALL, [0, 0], dtype=BF16, max_batch_per_device=SMALL_B)
    g.load_weights(blob)
    g.fill_inputs_seeded(1, SMALL_B)          # member i: seed 1 + i
    g.forward_resident(SMALL_B, steps=6)
    got = g.read_logits(SMALL_B)
    g.close()
    ctx = vithip.VitContext(SMALL, dtype=BF16, max_batch=SMALL_B)
    ctx.load_weights(blob)
    for i in range(2):
        want = ctx.forward(S.make_images(SMALL, 1 + i, SMALL_B))
        assert same_bits(got[i * SMALL_B:(i + 1) * SMALL_B], want), i
    ctx.close()

"""Seeded call sequences for the context model (tests/ctx_model.py): what test_ctx_model_host.py counts and
test_gpu_ctx_sequences.py runs.  The generator walks the model along, so it knows which calls the context must refuse and
provokes those on purpose; it imports nothing of the library."""
import copy
import random

import ctx_model as M

# (res_w, res_h, ssaa) -> the supersampled frame is (int(f32(res_w) * ssaa), int(f32(res_h) * ssaa)); all three values are exact
FRAMES = {
    "cornell": dict(scene="cornell_box", res=(40, 24), ssaa=1.0, nw=40, nh=24),
    "sink": dict(scene="kitchen_sink", res=(37, 23), ssaa=1.5, nw=55, nh=34),     # ragged against the 8x8 tiles
    "tiny": dict(scene="cornell_box", res=(16, 8), ssaa=1.0, nw=16, nh=8),        # the frame of the 1024-bookings sequences
}
BOUNCE = 4

VARIANTS = {
    "plain": dict(flags=0),
    "no_lookahead": dict(flags=M.FLAG_NO_LOOKAHEAD),
    "defer": dict(flags=M.FLAG_DEFER),
    "defer_no_lookahead": dict(flags=M.FLAG_DEFER | M.FLAG_NO_LOOKAHEAD),
    "count_segments": dict(flags=M.FLAG_COUNT_SEGMENTS),
    "shard": dict(flags=0, shard=(1, 3, 8)),
    "bound": dict(flags=0, bound=True),                     # bound to caller memory before the first call
    "k_split": dict(flags=0, env={"MRT_K_SPLIT": "4"}),     # the knob of test_sample_split_launch_is_bit_identical
}
SEEDS = tuple(range(12))

EXECUTE_N = (1, 1, 1, 1, 2, 3, 15, 16, 17, 33, 100)
OBSERVE = ("accum", "accum_local", "img", "img_ss", "img_hdr", "denoise", "sample_counts", "stats")
SYNTH_COUNTS = (3, 7, 21, 37, 50)                           # none a multiple of 16
ADAPTIVE = ((float("inf"), 32, 64, 16), (0.0, 32, 32, 16), ("median", 32, 64, 16))      # "median": the frame's own threshold
BUDGET = 300                                                # samples per sequence, about


def frame_of(seed):
    return "sink" if seed % 2 else "cornell"


def model_of(frame, variant):
    f, v = FRAMES[frame], VARIANTS[variant]
    sh = v.get("shard", (0, 1, 8))
    return M.Ctx(f["nw"], f["nh"], v["flags"], *sh)


def prefix_of(variant):
    return [("bind", "fit")] if VARIANTS[variant].get("bound") else []


def model_threshold(call):
    """The call as the model takes it: the frame's median threshold is some finite positive number."""
    return ("adaptive", 0.5) + tuple(call[2:]) if call[0] == "adaptive" and call[1] == "median" else call


def model_apply(m, call):
    """The model's status with stand-in tile counts where only the image can tell them (every tile at min_samples: the counts
    steer no later status, they are positive multiples of 32 either way)."""
    c = model_threshold(call)
    return m.apply(c, tile_counts=[c[2]] * (m.n_tx * m.n_ty) if c[0] == "adaptive" else None)


def generate(seed, variant):
    """20-40 draws from the alphabet (a burst of one-sample calls is one draw), every provoked refusal followed by an
    observation and half of them preceded by one, an observation at the end."""
    rng = random.Random(seed * 1009 + sorted(VARIANTS).index(variant))
    m = model_of(frame_of(seed), variant)
    calls = []
    used = 0
    n_slots = 0

    def emit(call):
        nonlocal used
        refused = model_apply(copy.deepcopy(m), call) != M.OK
        if refused and rng.random() < 0.5:
            calls.append(("accum",)); model_apply(m, ("accum",))
        calls.append(call)
        rc = model_apply(m, call)
        assert (rc != M.OK) == refused
        if rc == M.OK:
            used += {"execute": call[1] if call[0] == "execute" else 0, "burst": call[1] if call[0] == "burst" else 0,
                     "adaptive": 64 if call[0] == "adaptive" else 0}.get(call[0], 0)
        else:
            calls.append(("accum",)); model_apply(m, ("accum",))

    for c in prefix_of(variant):
        emit(c)
    if rng.random() < 0.35:                                 # an image before any sample
        emit((rng.choice(M.NEEDS_WHOLE_FRAME),))
    draws = rng.randint(20, 40)
    ones_left = 0
    burst_done = False
    while draws > 0:
        draws -= 1
        if ones_left:
            ones_left -= 1
            emit(("execute", 1))
            continue
        r = rng.random()
        after_ones = m.lookahead_live or m.pending > 0      # land the rarer calls where a run is live or samples are booked
        if m.adaptive is not None and r < 0.42:             # an adaptive render: most executes would only be refused
            sub = rng.random()
            if sub < 0.2:
                emit(("execute", rng.choice(EXECUTE_N)))
            elif sub < 0.45:
                door = rng.choice(("reset", "set_accum", "set_accum_device"))
                emit((door,) if door == "reset" else (door, ("synth", rng.randrange(1000), rng.choice(SYNTH_COUNTS))))
            else:
                emit((rng.choice(OBSERVE + ("adapt_half",)),))
        elif r < (0.25 if after_ones else 0.42):
            n = rng.choice(EXECUTE_N)
            if used + n > BUDGET:
                n = 1
            emit(("execute", n))
            if n == 1:
                ones_left = rng.choice((0, 2, 3, 3, 5, 9))
        elif r < 0.45 and not burst_done and m.adaptive is None and used + 48 <= BUDGET + 40:
            burst_done = True
            emit(("burst", rng.randint(40, 48)))
        elif r < 0.66:
            if rng.random() < 0.2:
                emit(("save", n_slots)); n_slots += 1
            else:
                emit((rng.choice(OBSERVE),))
        elif r < 0.71:
            emit(("reset",))
        elif r < 0.79:
            good = [k for k in range(n_slots) if m.slots[k] % 16]
            src = ("slot", rng.choice(good)) if good and rng.random() < 0.6 else ("synth", rng.randrange(1000), rng.choice(SYNTH_COUNTS))
            emit((rng.choice(("set_accum", "set_accum", "set_accum_device")), src))
        elif r < 0.835:
            emit(("bind", "small" if rng.random() < 0.3 else "fit"))
        elif r < 0.86:
            emit(("unbind",))
        elif r < 0.88:
            emit(("device_ptr",))
        elif r < 0.94:
            if rng.random() < 0.5 and not m.sharded and used + 64 <= BUDGET + 64:
                emit(("reset",))                            # make it legal
            emit(("adaptive",) + rng.choice(ADAPTIVE))
        elif r < 0.96:
            emit(("adapt_half",))
        else:
            emit((rng.choice(("radiance", "aov")),))
    emit(("stats",))
    emit(("accum",))
    return calls


# ---- hand-written sequences, next to the generated ones: (frame, variant, calls) ---------------------------------------------------
def _bookings_1030():
    return ([("execute", 1)] * 500 + [("aov",), ("radiance",)] + [("execute", 1)] * 530 + [("stats",), ("accum",), ("img",)] +
            [("execute", 1)] * 3 + [("reset",), ("accum",), ("execute", 1), ("sample_counts",)])


def _bookings_overshoot():
    """Bookings of n > 1 that overshoot 1024: the whole of what is booked goes out as one launch."""
    return ([("execute", 1)] * 1000 + [("execute", 17), ("execute", 33), ("stats",), ("execute", 2), ("img_hdr",), ("accum",)])


NAMED = {
    "bookings_1030": ("tiny", ("defer", "defer_no_lookahead"), _bookings_1030),
    "bookings_overshoot": ("tiny", ("defer",), _bookings_overshoot),
    # set_accum with a look-ahead set in flight; a refused adaptive call between two one-sample calls; a bind in mid-run
    "mid_run_replacements": ("cornell", ("plain", "defer", "k_split"), lambda: (
        [("execute", 1)] * 5 + [("save", 0)] + [("execute", 1)] * 4 + [("set_accum", ("slot", 0))] + [("execute", 1)] * 4 +
        [("adaptive", 0.0, 32, 32, 16), ("accum",)] + [("execute", 1)] * 3 + [("bind", "fit")] + [("execute", 1)] * 4 + [("accum",), ("unbind",)] +
        [("execute", 1)] * 4 + [("bind", "small"), ("accum",), ("reset",)] + [("execute", 1)] * 4 + [("device_ptr",), ("img",)] + [("execute", 1)] * 4 + [("accum",)])),
    # Found by mid_run_replacements: a bind after a restored run and an observation, then one-sample calls at once.  mrt_bind_accum
    # copied the accumulator over with a device-to-device hipMemcpy, which returns before the copy is done and runs on the null
    # stream; the fold of the next look-ahead plane read the new memory first, and the copy then wrote that sample away (about one
    # run in six).  The shortest sequence that showed it.
    "bind_then_one_sample_calls": ("cornell", ("plain", "k_split", "shard"), lambda: (
        [("execute", 1)] * 5 + [("save", 0)] + [("execute", 1)] * 4 + [("set_accum", ("slot", 0))] + [("execute", 1)] * 4 + [("accum",)] +
        [("execute", 1)] * 3 + [("bind", "fit")] + [("execute", 1)] * 4 + [("accum",)])),
}


def named_cases():
    return [(name, variant) for name, (_, variants, _) in NAMED.items() for variant in variants]


def named(name):
    frame, _, build = NAMED[name]
    return frame, build()

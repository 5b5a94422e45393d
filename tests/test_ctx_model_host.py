"""The context model (tests/ctx_model.py) and the sequence generator (tests/ctx_sequences.py) without a device: the model on
the scripts of the six hand-written state tests, whose outcomes those tests assert on the GPU, and the census of what the
committed seeds cover."""
import collections

import ctx_model as M
import ctx_sequences as Q

INF = float("inf")


def run(m, calls):
    return [m.apply(c) for c in calls]


def test_model_on_look_ahead_serves_the_per_call_loop_bit_for_bit():
    for flags in (0, M.FLAG_NO_LOOKAHEAD):
        m = M.Ctx(96, 64, flags)
        for i in range(45):
            assert m.lookahead_live == (flags == 0 and i >= 3)
            assert m.apply(("execute", 1)) == M.OK and m.apply(("accum",)) == M.OK and m.frame_count == i + 1
        assert m.log == [(i, 1) for i in range(45)] and m.stats_samples == 96 * 64
        run(m, [("execute", 19)])
        assert not m.lookahead_live
        run(m, [("execute", 1)] * 5 + [("save", 0)])
        assert m.frame_count == 69 and m.log[45:] == [(45, 19)] + [(64 + i, 1) for i in range(5)]
        run(m, [("reset",)] + [("execute", 1)] * 4 + [("set_accum", ("slot", 0))])
        assert m.restored == (("slot", 0), 69) and m.log == [] and not m.lookahead_live
        run(m, [("execute", 1)] * 6 + [("accum",)])
        assert m.frame_count == 75 and m.log == [(69 + i, 1) for i in range(6)] and m.epoch == 2


def test_model_on_deferred_execution_books_calls_and_traces_them_batched():
    d = M.Ctx(96, 64, M.FLAG_DEFER)
    assert run(d, [("execute", 1)] * 40) == [M.OK] * 40 and d.log == [] and d.pending == 40 and d.count == 0
    d.apply(("accum",))
    assert d.frame_count == 40 and d.log == [(0, 40)] and d.stats_samples == 96 * 64 * 40 and d.stats_deferred == 1
    assert d.apply(("img",)) == M.OK
    upd = M.Ctx(96, 64, M.FLAG_DEFER)                   # an image after every sample: the eager loop's log
    for i in range(6):
        assert run(upd, [("execute", 1), ("img",)]) == [M.OK, M.OK]
    assert upd.log == [(i, 1) for i in range(6)]
    big = M.Ctx(32, 24, M.FLAG_DEFER)
    run(big, [("execute", 1)] * 1100)
    assert big.log == [(0, 1024)] and big.pending == 76
    big.apply(("accum",))
    assert big.log == [(0, 1024), (1024, 76)] and big.frame_count == 1100
    run(big, [("execute", 1), ("reset",), ("accum",)])
    assert big.frame_count == 0 and big.log == [] and big.pending == 0 and big.pixel_counts()[23][31] == 0


def test_model_cuts_no_booking_at_1024():
    """Bookings of n > 1 that overshoot: everything booked goes out as one launch range (include/mrt.h, MRT_FLAG_DEFER)."""
    m = M.Ctx(16, 8, M.FLAG_DEFER)
    run(m, [("execute", 1)] * 1000 + [("execute", 17)])
    assert m.log == [] and m.pending == 1017
    m.apply(("execute", 33))
    assert m.log == [(0, 1050)] and m.pending == 0 and m.stats_samples == 128 * 1050 and m.stats_deferred == 1
    m.apply(("execute", 2))
    assert m.apply(("stats",)) == M.OK and m.log == [(0, 1050), (1050, 2)] and m.stats_samples == 128 * 2


def test_model_on_reset_and_set_accum_roundtrip():
    m = M.Ctx(64, 36)
    assert run(m, [("execute", 2), ("save", 0), ("img",), ("reset",), ("accum",)]) == [M.OK] * 5
    assert m.frame_count == 0 and m.log == [] and m.restored is None
    assert run(m, [("set_accum", ("slot", 0)), ("img",)]) == [M.OK, M.OK]
    assert m.frame_count == 2 and m.restored == (("slot", 0), 2) and m.log == []


def test_model_on_adaptive_state_rules():
    ad = ("adaptive", 0.05, 32, 64, 16)
    tiles = [32, 64] * 52                                # 100 x 60: 13 x 8 tiles
    m = M.Ctx(100, 60)
    assert m.apply(ad, tile_counts=tiles) == M.OK and m.frame_count == 32 and m.pixel_counts()[0][8] == 64
    assert m.stats_samples == sum(k * min(8, 100 - (t % 13) * 8) * min(8, 60 - (t // 13) * 8) for t, k in enumerate(tiles))
    assert run(m, [("execute", 4), ad, ("adapt_half",)]) == [M.ERR_STATE, M.ERR_STATE, M.OK]
    assert run(m, [("reset",), ("execute", 4), ("accum",), ("adapt_half",), ad]) == [M.OK, M.OK, M.OK, M.ERR_STATE, M.ERR_STATE]
    assert m.frame_count == 4 and m.pixel_counts()[59][99] == 4
    m.apply(("reset",))
    for bad in [dict(step=24), dict(step=0), dict(mn=48), dict(mn=0), dict(mx=80), dict(mn=128, mx=64), dict(thr=-1.0), dict(thr=float("nan"))]:
        kw = dict(thr=0.05, mn=32, mx=64, step=16)
        kw.update(bad)
        assert m.apply(("adaptive", kw["thr"], kw["mn"], kw["mx"], kw["step"])) == M.ERR_ARG, bad
    assert m.apply(ad, tile_counts=tiles) == M.OK        # nothing was changed by the refusals
    assert run(m, [("save", 0), ("set_accum", ("slot", 0)), ("execute", 1)]) == [M.OK] * 3 and m.adaptive is None and m.log == [(32, 1)]
    assert M.Ctx(100, 60, 0, 0, 2, 8).apply(ad, tile_counts=tiles) == M.ERR_STATE


def test_model_on_the_context_is_untouched():
    for flags, log, samples in ((0, [(0, 8), (8, 8)], 8), (M.FLAG_DEFER, [(0, 16)], 16)):
        a, b = M.Ctx(24, 16, flags), M.Ctx(24, 16, flags)
        run(a, [("execute", 8), ("radiance",), ("execute", 8), ("accum",), ("stats",)])
        run(b, [("execute", 8), ("execute", 8), ("accum",), ("stats",)])
        for m in (a, b):
            assert m.log == log and m.frame_count == 16 and m.stats_samples == 24 * 16 * samples and m.stats_deferred == int(flags != 0)


def test_model_on_booked_samples_are_traced_first():
    d = M.Ctx(24, 16, M.FLAG_DEFER)
    assert M.Ctx(24, 16, M.FLAG_DEFER).apply(("img_hdr",)) == M.ERR_STATE
    assert run(d, [("execute", 1), ("execute", 1), ("img_hdr",), ("stats",)]) == [M.OK] * 4
    assert d.stats_deferred == 1 and d.frame_count == 2 and d.log == [(0, 2)]


def test_model_exposed_memory_and_shards():
    d = M.Ctx(40, 24, M.FLAG_DEFER)
    assert run(d, [("execute", 3), ("bind", "small")]) == [M.OK, M.ERR_ARG] and d.log == [(0, 3)] and not d.bound      # traced first, then refused
    assert run(d, [("execute", 2), ("device_ptr",), ("execute", 1), ("unbind",), ("execute", 1)]) == [M.OK] * 5
    assert d.log == [(0, 3), (3, 2), (5, 1), (6, 1)] and d.stats_deferred == 0 and d.handed_out
    s = M.Ctx(55, 34, 0, 1, 3, 8)
    assert s.rows == list(range(8, 16)) + [32, 33] and s.padded_rows == 16
    assert run(s, [("execute", 2), ("img",), ("accum",), ("set_accum", ("synth", 1, 7)), ("img",), ("execute", 1)]) == [M.OK, M.ERR_STATE, M.OK, M.OK, M.OK, M.OK]
    assert s.frame_count == 7 and s.count == 3 and s.log == [(0, 2), (2, 1)] and s.stats_samples == 10 * 55
    s.apply(("reset",))
    assert s.full is None and s.frame_count == 0


# ---- the census -------------------------------------------------------------------------------------------------------------------
def census():
    c = dict(kinds=collections.Counter(), refusals=collections.Counter(), doors=collections.Counter(), live=collections.Counter(),
             booked=collections.Counter(), longest_run=0, crossed_1024=0, calls=0, sequences=0)
    seqs = [(Q.frame_of(seed), v, Q.generate(seed, v)) for v in Q.VARIANTS for seed in Q.SEEDS]
    seqs += [(Q.named(name)[0], v, Q.prefix_of(v) + Q.named(name)[1]) for name, v in Q.named_cases()]
    for frame, variant, calls in seqs:
        m = Q.model_of(frame, variant)
        c["sequences"] += 1
        run_len = 0
        for call in calls:
            kind = call[0]
            labels, was_adaptive, n_log = m.labels(), m.adaptive is not None, len(m.log)
            big_before = any(n >= M.DEFER_LIMIT for _, n in m.log)
            rc = Q.model_apply(m, call)
            c["calls"] += 1
            for lab in labels:
                c["kinds"][kind, lab] += 1
            if rc != M.OK:
                why = {"execute": "execute in adaptive mode", "adaptive": "adaptive on a sharded context" if m.sharded else "adaptive on a context with samples",
                       "adapt_half": "adapt_half without an adaptive call", "bind": "undersized bind_accum"}.get(kind)
                if kind in M.NEEDS_WHOLE_FRAME:
                    why = "image on a shard without set_accum" if m.sharded and not m.full else "image at count 0"
                c["refusals"][why, rc] += 1
            if kind in ("reset", "set_accum", "set_accum_device", "bind"):
                k = "set_accum" if kind == "set_accum_device" else kind
                c["live"][k] += "la_live" in labels
                c["booked"][k] += "booked" in labels
                if was_adaptive and m.adaptive is None:
                    c["doors"][kind] += 1
            one = kind == "burst" or call == ("execute", 1)
            run_len = run_len + (call[1] if kind == "burst" else 1) if one and rc == M.OK else 0
            c["longest_run"] = max(c["longest_run"], run_len)
            if not big_before and any(n >= M.DEFER_LIMIT for _, n in m.log[n_log:]):
                c["crossed_1024"] += 1
    return c


LABELS = ("uniform", "adaptive", "la_live", "booked", "bound", "handed_out", "owned")


def possible(kind, label):
    """Every call kind in every state, but a burst on an adaptive render: that is forty refusals of ("execute", 1), which occurs."""
    return (kind, label) != ("burst", "adaptive")


def test_sequences_cover_what_they_claim():
    c = census()
    print(f"{c['sequences']} sequences, {c['calls']} calls; longest run of one-sample calls {c['longest_run']}; 1024 crossed {c['crossed_1024']} times")
    print("refusals:", dict(c["refusals"]))
    print("adaptive -> uniform:", dict(c["doors"]), " with a look-ahead run live:", dict(c["live"]), " with samples booked:", dict(c["booked"]))
    missing = [(k, lab) for k in M.KINDS for lab in LABELS if possible(k, lab) and not c["kinds"][k, lab]]
    print("rarest (kind, state):", sorted((n, k) for k, n in c["kinds"].items())[:5])
    assert not missing, missing
    want = [("image at count 0", M.ERR_STATE), ("execute in adaptive mode", M.ERR_STATE), ("adaptive on a context with samples", M.ERR_STATE),
            ("adaptive on a sharded context", M.ERR_STATE), ("adapt_half without an adaptive call", M.ERR_STATE),
            ("image on a shard without set_accum", M.ERR_STATE), ("undersized bind_accum", M.ERR_ARG)]
    assert set(c["refusals"]) == set(want) and all(c["refusals"][w] >= 3 for w in want), c["refusals"]
    assert c["longest_run"] >= 40
    assert all(c["live"][k] >= 1 and c["booked"][k] >= 1 for k in ("reset", "set_accum", "bind")), (c["live"], c["booked"])
    assert all(c["doors"][k] >= 1 for k in ("reset", "set_accum", "set_accum_device")), c["doors"]
    assert c["crossed_1024"] >= 2

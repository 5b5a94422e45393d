"""A state model of one mrt_ctx, written from the text of include/mrt.h (and DESIGN.md §9, §12) alone: for any sequence of
calls it says what every call returns and what the context then holds, without looking at the code under test.  It imports
nothing of the library and nothing but the standard library.

Three facts make that possible (include/mrt.h): the image is a pure function of (scene, seed, sample index); a launch over
the samples [base, base + n) adds the sums of its aligned 16-sample chunks, each summed from 0, to the accumulator in chunk
order; and the header says what each call does to the count, the mode and the accumulator.  So the accumulator's bits are
fixed by what it was last set to -- zero (mrt_create, mrt_reset, mrt_execute_adaptive) or a restored frame (mrt_set_accum*) --
and by the ordered list of launches folded into it since: the LOGICAL LAUNCH LOG.  A plain context fed those contents and
those launches must hold the same bits, and the oracle the same means.

Calls are tuples:
    ("execute", n)                      mrt_execute(n)
    ("burst", k)                        k consecutive mrt_execute(1)
    ("accum",) ("accum_local",) ("img",) ("img_ss",) ("img_hdr",) ("denoise",) ("sample_counts",) ("stats",)
    ("save", slot)                      mrt_accum whose frame and count the caller keeps in `slot`
    ("reset",)
    ("set_accum", src) ("set_accum_device", src)     src: ("slot", k) -- the frame kept there, at its count -- or
                                        ("synth", seed, count) -- a synthetic frame
    ("bind", "fit" | "small")           mrt_bind_accum of a buffer of exactly the needed size / one float short of it
    ("unbind",)                         mrt_bind_accum(ctx, NULL, 0)
    ("device_ptr",)                     mrt_accum_device_ptr
    ("adaptive", threshold, min_samples, max_samples, step)
    ("adapt_half",)
    ("radiance",) ("aov",)              change nothing
"""
import math

OK, ERR_ARG, ERR_STATE = 0, -1, -5
FLAG_COUNT_SEGMENTS, FLAG_DEFER, FLAG_NO_LOOKAHEAD = 1, 4, 8
CHUNK = 16
DEFER_LIMIT = 1024

OBSERVATIONS = ("accum", "accum_local", "img", "img_ss", "img_hdr", "denoise", "sample_counts", "stats", "save")
NEEDS_WHOLE_FRAME = ("img", "img_ss", "img_hdr", "denoise")         # ... and at least one sample
SETTLES = OBSERVATIONS + ("set_accum", "set_accum_device", "bind", "unbind", "device_ptr")
UNTOUCHED = ("radiance", "aov")
KINDS = ("execute", "burst") + OBSERVATIONS + ("reset", "set_accum", "set_accum_device", "bind", "unbind", "device_ptr", "adaptive",
                                                "adapt_half") + UNTOUCHED


def shard_rows_of(nh, shard_index, shard_count, shard_rows):
    """Frame rows of one shard: rows are dealt in blocks of shard_rows (at most nh) rows, block b to shard b % shard_count."""
    if shard_count <= 1:
        return list(range(nh))
    rows = min(shard_rows or 8, nh)
    return [y for y in range(nh) if (y // rows) % shard_count == shard_index]


def padded_rows_of(nh, shard_count, shard_rows):
    if shard_count <= 1:
        return nh
    rows = min(shard_rows or 8, nh)
    return -(-(-(-nh // rows)) // shard_count) * rows


class Ctx:
    def __init__(self, nw, nh, flags=0, shard_index=0, shard_count=1, shard_rows=8):
        self.nw, self.nh, self.flags = nw, nh, flags
        self.shard_count = max(1, shard_count)
        self.rows = shard_rows_of(nh, shard_index, self.shard_count, shard_rows)
        self.padded_rows = padded_rows_of(nh, self.shard_count, shard_rows)
        self.n_tx, self.n_ty = -(-nw // 8), -(-nh // 8)
        self.defer = bool(flags & FLAG_DEFER)
        # look-ahead serves eager one-sample calls only; MRT_FLAG_COUNT_SEGMENTS implies MRT_FLAG_NO_LOOKAHEAD
        self.lookahead = not (flags & (FLAG_DEFER | FLAG_COUNT_SEGMENTS | FLAG_NO_LOOKAHEAD)) and bool(self.rows)
        self.count = 0                  # the context's own sample count (adaptive: the smallest per-tile count)
        self.pending = 0                # samples booked under MRT_FLAG_DEFER
        self.bound = False              # mrt_bind_accum: the accumulator lives in caller memory
        self.handed_out = False         # mrt_accum_device_ptr gave the pointer away (for good)
        self.adaptive = None            # per-tile counts [n_ty * n_tx] of the adaptive render the context holds
        self.restored = None            # (src, count) the accumulator was last restored from; None: it was last zeroed
        self.log = []                   # the logical launch log since then: [(base, n)]
        self.epoch = 0                  # goes up whenever the accumulator is zeroed or restored: log and restored start over
        self.full = None                # a sharded context: (src, count) of the whole frame it received, kept next to its own rows
        self.slots = {}                 # slot -> count of the frame saved there
        self.ones = 0                   # consecutive eager one-sample calls
        self.stats_samples = 0
        self.stats_deferred = 0

    # ---- what the header derives from the state ----------------------------------------------------------------------------
    @property
    def sharded(self):
        return self.shard_count > 1

    @property
    def exposed(self):
        return self.bound or self.handed_out

    @property
    def lookahead_live(self):
        """Samples are traced ahead: from the third consecutive eager one-sample call on."""
        return self.lookahead and self.ones >= 3

    @property
    def frame_count(self):
        """*count of mrt_accum: the count of the frame the observations read."""
        return self.full[1] if self.full else self.count

    def pixel_counts(self):
        """counts[nh][nw] of mrt_sample_counts."""
        if self.adaptive is None:
            return [[self.frame_count] * self.nw for _ in range(self.nh)]
        return [[self.adaptive[(y // 8) * self.n_tx + x // 8] for x in range(self.nw)] for y in range(self.nh)]

    def labels(self):
        """The corners of the state space a call arrives in (test_sequences_cover_what_they_claim)."""
        out = {"adaptive" if self.adaptive is not None else "uniform"}
        if self.lookahead_live: out.add("la_live")
        if self.pending: out.add("booked")
        if self.bound: out.add("bound")
        if self.handed_out: out.add("handed_out")
        if not self.exposed: out.add("owned")
        if self.full: out.add("full_frame_on_shard")
        return out

    # ---- the launch log ----------------------------------------------------------------------------------------------------
    def _trace(self, n):
        self.log.append((self.count, n))
        self.count += n
        self.stats_samples = len(self.rows) * self.nw * n

    def _settle(self):
        if self.pending:
            n, self.pending = self.pending, 0
            self._trace(n)          # everything booked, as ONE launch range

    def _execute(self, n):
        if self.adaptive is not None:
            return ERR_STATE
        if self.defer and not self.exposed:
            self.pending += n
            if self.pending >= DEFER_LIMIT:
                self._settle()      # the whole of what is booked, the call that crossed 1024 included: no cut at 1024
            self.stats_deferred = 1
        else:
            self.ones = self.ones + 1 if n == 1 else 0
            self._trace(n)          # (look-ahead: the plain loop's bits, so the plain loop's log)
            self.stats_deferred = 0
        return OK

    def _zeroed_or_restored(self, restored):
        self.epoch += 1
        self.restored, self.log, self.adaptive, self.ones = restored, [], None, 0

    def _src_count(self, src):
        return self.slots[src[1]] if src[0] == "slot" else src[2]

    # ---- one call ----------------------------------------------------------------------------------------------------------
    def apply(self, call, tile_counts=None):
        """The status the call returns; the state moves as the header says.  A refused call changes no state, except that an
        entry point that traces booked samples first does so before it refuses (the samples are the same, the launch log is
        not).  tile_counts: the per-tile stop counts of an adaptive call whose threshold makes them depend on the image."""
        kind = call[0]
        if kind == "execute":
            return self._execute(call[1])
        if kind == "burst":
            rc = OK
            for _ in range(call[1]):
                rc = self._execute(1)
            return rc
        if kind in UNTOUCHED:
            return OK
        if kind == "adapt_half":
            return OK if self.adaptive is not None else ERR_STATE
        if kind == "reset":
            self.pending = 0        # booked samples are dropped with everything else
            self.count, self.full = 0, None
            self._zeroed_or_restored(None)
            return OK
        if kind == "adaptive":
            _, thr, mn, mx, step = call
            if step == 0 or step % CHUNK or mn == 0 or mx == 0 or mn % (2 * step) or mx % (2 * step) or mn > mx or not thr >= 0:
                return ERR_ARG
            if self.sharded or self.adaptive is not None or self.count or self.pending or self.full:
                return ERR_STATE
            n_tiles = self.n_tx * self.n_ty
            if mn == mx or thr == math.inf:
                tiles = [mn] * n_tiles
            else:
                tiles = list(tile_counts)
                assert len(tiles) == n_tiles and all(mn <= t <= mx and (t - mn) % (2 * step) == 0 for t in tiles)
            self._zeroed_or_restored(None)
            self.adaptive = tiles
            self.count = min(tiles)
            px = lambda t: min(8, self.nw - (t % self.n_tx) * 8) * min(8, self.nh - (t // self.n_tx) * 8)
            self.stats_samples = sum(k * px(t) for t, k in enumerate(tiles))
            self.stats_deferred = 0
            return OK
        assert kind in SETTLES, call
        self._settle()
        if kind in ("set_accum", "set_accum_device"):
            cnt = self._src_count(call[1])
            self.ones = 0
            if self.sharded:
                self.adaptive = None
                self.full = (call[1], cnt)          # next to the shard's own rows, which go on as they were
            else:
                self.count = cnt
                self._zeroed_or_restored((call[1], cnt))
            return OK
        if kind == "bind":
            if call[1] == "small":
                return ERR_ARG
            self.bound = True
            return OK
        if kind == "unbind":
            self.bound = False
            return OK
        if kind == "device_ptr":
            self.handed_out = True
            return OK
        if kind in NEEDS_WHOLE_FRAME:
            if (self.sharded and not self.full) or self.frame_count == 0:
                return ERR_STATE
            return OK
        if kind == "save":
            self.slots[call[1]] = self.frame_count
        return OK

"""Range guard of the trunk's reduced-range activation formats (include/mmmot_hip.h: mmmot_trunk_range_read).

The hq8 / hl16 activation formats have a finite range: e4m3 copies saturate above 1792 (products of that element become
fp16-class), the fp16 `hi` half clamps at 65000 (wrong value).  The trunk epilogues count both on the device; the guard
reads the counters synchronously on its engine's first forward (and repeats that forward's trunk when they are hit),
asynchronously after every later one (a 16-byte read-back inspected at the next forward: no synchronisation, one step
of lag), and moves the engine's trunk f16q8 -> f16x3 -> f32 for good.  MMMOT_RANGE_CHECK_EVERY=n adds a synchronous
check-and-recompute every n forwards; MMMOT_RANGE_GUARD=0 disables the guard.  See RangeGuard.run.

One ``RangeGuard`` belongs to one ``Engine`` and reaches `trunk`, `q8_in_force`, `trunk_elements`, `ops` and the
engine's lock through it, at call time.  What it finds it writes to the engine, where callers look for it:
`range_events`, `out_of_range_window`, `last_out_of_range_forward` and the lowered `trunk`.
"""
import os
import warnings

import torch


class RangeGuard:
    def __init__(self, engine):
        self.engine = engine
        self.enabled = os.environ.get('MMMOT_RANGE_GUARD', '1') != '0'
        self.check_every = int(os.environ.get('MMMOT_RANGE_CHECK_EVERY', '0'))
        self.q8_sat_limit = float(os.environ.get('MMMOT_Q8_SAT_LIMIT', '1e-4'))  # tolerated fraction of saturated elements
        self.n_forward = 0  # trunk runs under run() so far: "forward k of this engine" is the k-th of them, from 0
        self.block = self.host = self.pending = None  # counter block, its host mirror, queued read-back (event, first, last)
        self.seen = [0, 0, 0]  # counter values already accounted for (the block is cumulative)
        self.win0 = 0  # first forward whose trunk launches no inspected / queued read-back covers yet
        self.plan = None  # plan of the latest guarded trunk (settle judges the counters against it)

    def _block(self, dev):
        """this guard's own counter block (int32 [4] on `dev`) + its host mirror"""
        dev = torch.device(dev)
        if self.block is None or self.block.device != dev:
            self.block = torch.zeros(4, dtype=torch.int32, device=dev)
            self.host = torch.zeros(4, dtype=torch.int32)
            if dev.type == 'cuda':
                self.host = self.host.pin_memory()
            self.pending = None
            self.seen = [0, 0, 0]
        return self.block

    def read(self, reset=True):
        """Synchronous read of the counters: (e4m3-saturated, fp16-clamped, conv1_1 hits) since the last reset.  One
        stream synchronisation; GraphedForward.check_range() is the caller for captured forwards."""
        if self.block is None:
            return 0, 0, 0
        v = [int(x) & 0xFFFFFFFF for x in self.block.cpu().tolist()[:3]]
        d = [(a - b) & 0xFFFFFFFF for a, b in zip(v, self.seen)]
        if reset:
            self.seen = v
        return d[0], d[1], d[2]

    def _verdict(self, plan, sat, clamp, c11, window):
        """arithmetic the counters call for (None: the current one holds)"""
        eng = self.engine
        q8 = eng.q8_in_force(plan.S)
        if clamp > 0 or (c11 > 0 and not q8):
            return 'f32'
        if q8 and (sat > self.q8_sat_limit * eng.trunk_elements(plan) * window or c11 > 0):
            return 'f16x3'
        return None

    def _event(self, plan, lower, sat, clamp, c11, recomputed, window=None):
        # `affected_forwards` = (first, last): indices (count of forwards of this engine, from 0) of the forwards whose
        # trunk launches the counters that tripped cover.  recomputed=True: one forward, the current one, and its results
        # were recomputed in the lowered arithmetic before they were returned.  False (asynchronous read-back): a read-back
        # is recorded behind forward k and inspected once its copy has completed - possibly several forwards later, and no
        # new one is queued meanwhile - so it covers every forward since the previous read-back up to k, NOT "the previous
        # forward": `window` carries exactly that range, stored with the pending copy when it was recorded.
        # Those results were ALREADY RETURNED: the caller discards / repeats the forwards first .. last
        # (the index of a result's forward = the value of `n_forward - 1` after the call; the engine's
        # `last_out_of_range_forward` = last and `out_of_range_window` = (first, last) keep the latest detection, None
        # while there was none).  `affected_forward` (the last index of the range) is kept for callers of the round-3
        # interface.
        eng = self.engine
        if recomputed or window is None:
            window = (self.n_forward, self.n_forward)
        ev = dict(forward=self.n_forward, affected_forward=window[1], affected_forwards=tuple(window), was=eng.trunk,
                  now=lower, e4m3_saturated=sat, fp16_clamped=clamp, conv1_1_hits=c11,
                  trunk_elements=eng.trunk_elements(plan), recomputed=recomputed)
        eng.range_events.append(ev)
        if not recomputed:
            eng.last_out_of_range_forward = window[1]
            eng.out_of_range_window = tuple(window)
        # stacklevel: _event <- run / _inspect_pending / _check_window <- ... the engine's or the model's frame
        warnings.warn('mmmot_amd range guard: trunk arithmetic %(was)s -> %(now)s (%(e4m3_saturated)d activation '
                      'elements beyond the e4m3 range, %(fp16_clamped)d beyond the fp16 range, of %(trunk_elements)d '
                      'per forward); ' % ev + ('the trunk of this forward is recomputed' if recomputed else
                                               'detected late: forwards %d..%d of this engine ran out of range and were '
                                               'already returned' % tuple(window)),
                      RuntimeWarning, stacklevel=4)
        eng.trunk = lower

    def run(self, launch, plan, crops, cat):
        """launch(plan, crops, cat) - the engine's trunk launch sequence - under the guard; inside the engine's lock.
        Every guard owns its counter block (bound around its trunk launches: mmmot_trunk_range_bind), so engines sharing
        a device and captured graphs never mix windows.  First forward: synchronous check, the trunk is launched again
        in the lowered arithmetic when it trips.  Every later forward: the 16-byte block is copied to pinned host memory
        behind the trunk (asynchronous) and inspected at the start of the NEXT forward - no synchronisation, detection
        lags by one step (the event says so); `check_every` > 0 adds a synchronous check-and-recompute every that many
        forwards.  Never inside a hipGraph capture: GraphedForward.check_range() reads the block of a captured forward."""
        eng = self.engine
        ops = eng.ops
        dev = crops.device
        capturing = torch.cuda.is_current_stream_capturing() if crops.is_cuda else False
        active = self.enabled and hasattr(ops, 'trunk_range_bind')
        if not active:
            launch(plan, crops, cat)
            self.n_forward += 1
            return
        blk = self._block(dev)
        first = self.n_forward == 0
        guard = eng.trunk != 'f32' and not capturing
        # ---- verdict of the previous forward's asynchronous read-back -------------------------------------------
        if guard and self.pending is not None and self._inspect_pending(plan):
            guard = eng.trunk != 'f32'
        sync = guard and (first or (self.check_every > 0 and self.n_forward % self.check_every == 0))
        if sync:
            # open the window of this forward.  What the counters hold at this point belongs to the forwards since the last
            # inspected read-back (an asynchronous copy that had not completed when this check came round is superseded
            # by this synchronous read): they get their verdict and event here instead of being dropped
            self._check_window(plan)
            sync = eng.trunk != 'f32'  # lowered to the exact arithmetic: nothing left to check
        self.plan = plan
        ops.trunk_range_bind(blk)
        try:
            launch(plan, crops, cat)
            while sync and eng.trunk != 'f32':
                sat, clamp, c11 = self.read(reset=True)
                lower = self._verdict(plan, sat, clamp, c11, 1)
                if lower is None:
                    break
                self._event(plan, lower, sat, clamp, c11, recomputed=True)
                launch(plan, crops, cat)
        finally:
            ops.trunk_range_bind(None)
        if guard and not sync and eng.trunk != 'f32' and self.pending is None:
            # stream-ordered: copy the (cumulative) block out and mark the point - inspected by the next forward
            self.host.copy_(blk, non_blocking=True)
            e = True
            if dev.type == 'cuda':
                e = torch.cuda.Event()
                e.record()
            # the counters are cumulative: this copy covers the forwards since the previous read-back up to this one
            self.pending = (e, self.win0, self.n_forward)
            self.win0 = self.n_forward + 1
        elif sync:
            self.win0 = self.n_forward + 1  # checked (and, if need be, recomputed) synchronously
        self.n_forward += 1

    def _inspect_pending(self, plan):
        """Verdict of the queued asynchronous read-back once its copy has completed (no synchronisation).  Returns
        True when it was inspected."""
        ev, w0, w1 = self.pending
        if not (ev is True or ev.query()):
            return False
        self.pending = None
        v = [int(x) & 0xFFFFFFFF for x in self.host.tolist()[:3]]
        sat, clamp, c11 = [(a - b) & 0xFFFFFFFF for a, b in zip(v, self.seen)]
        self.seen = v
        lower = self._verdict(plan, sat, clamp, c11, w1 - w0 + 1)
        if lower is not None:
            self._event(plan, lower, sat, clamp, c11, recomputed=False, window=(w0, w1))
        return True

    def _check_window(self, plan):
        """Synchronous verdict on the counters of every trunk launch since the last inspected read-back (one 16-byte
        read, which synchronises the stream); an event for those forwards when they left the range."""
        sat, clamp, c11 = self.read(reset=True)
        w0, w1 = self.win0, self.n_forward - 1
        if self.pending is not None:  # the copy that did not complete: its forwards are in these counters too
            w0 = min(w0, self.pending[1])
        self.pending = None
        if w1 >= w0:
            lower = self._verdict(plan, sat, clamp, c11, w1 - w0 + 1)
            if lower is not None:
                self._event(plan, lower, sat, clamp, c11, recomputed=False, window=(w0, w1))
        self.win0 = self.n_forward

    def settle(self, upto=None):
        """The guard's verdict on its engine's trunk launches up to forward `upto` (default: all so far) now, not at a
        later forward; takes the engine's lock, so not from inside a forward.  A queued read-back that covers `upto` is
        waited for and inspected (free once the caller has read that forward's results); forwards no read-back covers yet
        are judged by a synchronous read of the counter block; forwards already judged cost nothing.
        TrackingNet.appearance_is_current calls it for the forward that made the rows, so rows from an out-of-range trunk
        are recomputed before they are reused."""
        eng, plan = self.engine, self.plan
        if (plan is None or not self.enabled or self.block is None or eng.trunk == 'f32'
                or not hasattr(eng.ops, 'trunk_range_bind')):
            return
        upto = self.n_forward - 1 if upto is None else min(int(upto), self.n_forward - 1)
        with eng._exclusive():
            pend = self.pending
            if pend is not None and pend[1] <= upto <= pend[2]:
                if pend[0] is not True:
                    pend[0].synchronize()
                self._inspect_pending(plan)
            elif upto >= self.win0:
                self._check_window(plan)

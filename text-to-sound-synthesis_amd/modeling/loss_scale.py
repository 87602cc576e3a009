"""Loss-scale policy of the "f16x2" training backend: the host arithmetic around the calibrated scales (modeling/train.py).

The backward splits every GEMM operand to fp16 under a loss scale 2^k plus one power of two per site (train.py's module
docstring).  `TrainStep.calibrate` measures, this class decides: where a calibration aims (`_target`, `_exp_from_amax`,
`site_exponents`, `fwd_exponents`), when the calibrated scales are dropped again (`check_loss_scale`: the saturation monitor;
`observe_grad_norm`: the gradient norm), and what a weight swap or a re-capture forgets (`reset`).  Nothing here launches a
kernel of the library's; the only device objects are the monitors' scalars `_amax_live` (gradient side) and `_fwd_live` (forward side), which
the step's packs fold into and `check_loss_scale` reads with one host sync.

The FORWARD operands (LayerNorm outputs, attention outputs, gelu2(fc1 output)) are split unscaled as long as they stay under
2^13; a linear whose input has grown past that -- fc2's, on trained weights, is the one that gets there -- is packed under a
power of two 2^f <= 1 of its own (`fwd_exponents`, from the first calibration pass), taken out again by the forward epilogue
and the dW epilogue.  The split saturates silently at 65504, so real passes fold max |X 2^f| into `_fwd_live` and a reading at
or above the window's upper end drops the calibration like a gradient-side one.
"""
import math


class LossScalePolicy:
    def __init__(self, enabled=True):
        """enabled=False: the "fp32" backend -- `loss_scale_exp` is 0 for ever and every check answers False."""
        self.enabled = enabled
        self.loss_scale_exp = None if enabled else 0    # k of the loss scale 2^k; None: calibrate first
        self._site_exp = None                   # {linear key: e}: the site's own 2^e on top of the loss scale (calibrate)
        self._calib_norm = None                 # global gradient norm at calibration time (observe_grad_norm)
        self.last_trip = None                   # why the calibration was dropped last (text; a re-capture's reason)
        self._last_loss = None                  # the step's latest loss (device scalar): tells zero gradients from NaN ones
        # Saturation monitor of the split backend (ds_split_hi / _lo SATURATE at 65504 -- no inf / NaN ever shows that a
        # gradient left the calibrated window): every step folds max |scaled dY| over all GEMM inputs into this device
        # scalar (ds_amax, the calibration's own probe; captured into the graph like any other launch), and
        # check_loss_scale() reads it on the host every `monitor_interval` steps -- whether or not clipping is configured.
        self._amax_live = None
        # ... and the same for the forward operands: {linear key: f <= 0} of the last calibration (None: none yet; every
        # missing key is 0) and the device scalar the forward packs fold max |X 2^f| into (None until a step has run: the
        # host tests of this class leave it out)
        self.fwd_exp = None
        self._fwd_live = None
        self.monitor_interval = 16
        # Where a calibration puts the largest value of every fp16-split gradient operand of ITS batch: 2^calib_log2 .. 2x that.
        # What matters for precision is only that a tensor's largest element is >= 2^0 (a split value keeps 22 bits down to
        # 2^-3 and 2^-25 absolutely under that: with the maximum at 2^T every element errs by <= 2^-(25+T) of it -- fp32's own
        # 2^-24 at T = 0), and since round 6 EVERY site has its own power of two (calibrate: `_site_exp`), so the target can sit
        # low and leave the room above to the batches: rounds 3-5 put ONE global maximum at 2^12, three bits under the window's
        # upper bound, and the measured batch-to-batch spread of that maximum is three bits (most batches 2^-8.7, every fifth
        # 2^-5.73 = (1 / pt) / (B L): one position whose d logit is ~1) -- a run re-captured as soon as its first large batch
        # came by (profiles/r05last_monitor_ab.txt); per site the spread is another 2.5 bits (profiles/r06b_*).  6 leaves nine.
        self.calib_log2 = 6
        self.monitor_window = (0, 15)           # log2 bounds of max |scaled operand| outside which the calibration is dropped
        self.monitor_log = []                   # log2 of the last readings (host floats; tools/bench_train.py prints them)
        # what a HIGH reading teaches: by how many bits later calibrations aim lower (a calibration looks at ONE batch; the
        # excursion that tripped the monitor is then put at 2^12).  Forgotten after `cap_decay_readings` quiet readings in a
        # row, when a reading falls under the window, and when the weights are replaced.
        self._target_drop = 0
        self._clean_readings = 0                # consecutive readings under 2^11 while a drop is in force
        self.cap_decay_readings = 32            # ... after that many (512 iterations) the drop is forgotten
        self._since_check = 0
        # A calibration has seen ONE batch: the monitor is read after 1, 2, 4, 8 iterations before it settles at every
        # `monitor_interval`-th -- on trained-like weights a batch 2^11 above the calibration batch came by within the first 16
        # iterations (profiles/r06k_bench_train_long_runs.txt: reading 2^17.65, i.e. saturated planes until the check)
        self._next_check = 1

    def reset(self, weights_replaced=True):
        """The policy's share of TrainStep.reset_scales: the calibrated scales go; what the monitor had learnt about the OLD
        weights' gradients (`_target_drop`) goes with replaced weights only."""
        if weights_replaced:
            self._target_drop, self._clean_readings = 0, 0
        if self.enabled:
            self.loss_scale_exp = None
            self._site_exp = None
            self.fwd_exp = None
        self._calib_norm = None
        for live in (self._amax_live, self._fwd_live):
            if live is not None:
                live.zero_()

    def begin_calibration(self):
        """A calibration starts from the bare gradients (no scale at all) and restarts the monitor's 1, 2, 4, 8 schedule."""
        self.loss_scale_exp, self._site_exp, self.fwd_exp = 0, None, None
        self._next_check, self._since_check = 1, 0

    def check_loss_scale(self, force=False):
        """Host side of the saturation monitor: every `monitor_interval` calls (after 1, 2, 4, 8 calls right behind a
        calibration; or when forced) read max |scaled operand| over all sites since the last check (one sync) and drop the
        calibration when it has left `monitor_window` = [2^0, 2^15) -- fp16 saturates at 2^16, and a site whose largest element
        is under 2^0 no longer has fp32-class planes.  Returns True when the next step must re-calibrate (a captured iteration
        must then be re-captured)."""
        if not self.enabled or self._amax_live is None:
            return False
        self._since_check += 1
        if not force and self._since_check < min(self._next_check, self.monitor_interval):
            return False
        self._since_check = 0
        self._next_check = min(self.monitor_interval, 2 * self._next_check)
        if self._fwd_live is None:
            m, mf = float(self._amax_live.item()), 0.0
        else:                                   # both monitors in the one host sync
            import torch
            m, mf = torch.cat((self._amax_live.reshape(1), self._fwd_live.reshape(1).to(self._amax_live.device))).tolist()
            self._fwd_live.zero_()
        self._amax_live.zero_()
        self.monitor_log = self.monitor_log[-63:] + [round(math.log2(m), 2) if m > 0.0 and math.isfinite(m) else m]
        if not mf < 2.0 ** self.monitor_window[1]:
            # a forward operand has outgrown the power of two it was calibrated under (or never had one): its planes are
            # within a bit of saturating, or have.  The next calibration measures the forward again.
            self.last_trip = "forward operand high: max |X 2^f| = " + ("2^%.2f" % math.log2(mf) if math.isfinite(mf) else repr(mf))
            self.loss_scale_exp, self._calib_norm, self.fwd_exp = None, None, None
            return True
        if m == 0.0:
            # ds_amax never lets a NaN win and skips non-positive values, so 0 means EITHER genuinely zero gradients (nothing
            # was scaled: no reason to re-calibrate / re-capture) OR an all-NaN scaled dY (a diverged loss).  The loss of the
            # same step tells them apart at this very host sync.
            last = self._last_loss
            if last is not None and not math.isfinite(float(last)):
                # a diverged run: no loss scale repairs it, and answering True here would re-calibrate (and re-capture a graphed
                # iteration) at every monitor interval for the rest of the run
                raise FloatingPointError("training diverged: the loss is %r (every scaled gradient is NaN)" % float(last))
            return False
        lo, hi = self.monitor_window
        if math.isfinite(m) and 2.0 ** lo <= m < 2.0 ** hi:
            # inside the window.  What one excursion taught must not hold the target down for ever: once the readings have
            # stayed under 2^11 for `cap_decay_readings` checks in a row it is forgotten (the scales themselves are left
            # alone -- the next re-calibration, whenever something asks for one, aims at the full target again)
            if self._target_drop:
                self._clean_readings = self._clean_readings + 1 if m < 2.0 ** 11 else 0
                if self._clean_readings >= self.cap_decay_readings:
                    self._target_drop, self._clean_readings = 0, 0
            return False
        if math.isfinite(m) and m >= 2.0 ** hi:
            # put THIS excursion at 2^12 from now on: aim that many bits lower (never under 2^1)
            self._target_drop = min(self.calib_log2 - 1, self._target_drop + math.floor(math.log2(m)) - 12)
            self._clean_readings = 0
            self.last_trip = "monitor high: max |scaled operand| = 2^%.2f" % math.log2(m)
        elif math.isfinite(m):
            self._target_drop = 0                                              # gradients have shrunk: aim at the full target again
            self.last_trip = "monitor low: max |scaled operand| = 2^%.2f" % math.log2(m)
        else:
            self.last_trip = "monitor: max |scaled operand| = %r" % m
        self.loss_scale_exp, self._calib_norm = None, None
        return True

    def _target(self):
        """log2 of where calibrations put a site's largest operand value right now (calib_log2 minus what excursions taught)"""
        return max(1, self.calib_log2 - self._target_drop)

    def _exp_from_amax(self, m):
        """exponent k that puts a largest value m at 2^target .. 2^(target + 1)"""
        if m == 0.0 or not math.isfinite(m):
            return 0
        return self._target() - math.floor(math.log2(m))

    def site_exponents(self, keys, per_site):
        """{key: e} from the second calibration pass: max |operand| per site (under the loss scale, in the order the backward
        visits the sites) -> the power of two that puts it at the target, within 2^-40 .. 2^40"""
        return {k: max(-40, min(40, self._exp_from_amax(v))) for k, v in zip(keys, per_site)}

    @staticmethod
    def fwd_exponents(keys, per_site):
        """{key: f} from the first calibration pass: max |forward operand| per linear -> f = min(0, 12 - floor(log2 m)), the
        power of two that brings a maximum of 2^13 or more back to [2^12, 2^13) -- three bits under the monitor's 2^15, and
        inside the range (>= 2^-3 for everything within 2^15 of the maximum) where the split is fp32-class.  Never a shift up:
        below 2^13 an operand is split as it is (f = 0: the step's arithmetic to the bit).  0 for 0 / inf / NaN."""
        return {k: 0 if not (m > 0.0 and math.isfinite(m)) else min(0, 12 - math.floor(math.log2(m))) for k, m in zip(keys, per_site)}

    def observe_grad_norm(self, norm):
        """Second guard of the calibrated scales ("f16x2" backend, eager solver): the calibration leaves 2^9 of headroom below
        fp16's range and 2^6 above the point where the largest element of an operand would fall under 2^0.  Gradients grow and
        shrink together, so the global gradient norm the solver computes anyway is a monitor too: once it has moved by more
        than 32x up or 64x down from its value at calibration time, the next step re-calibrates (returns True then).  Call
        it with a HOST float (the solvers do, next to float(loss))."""
        if not self.enabled or not math.isfinite(norm) or norm <= 0.0:
            return False
        if self._calib_norm is None:
            self._calib_norm = norm
            return False
        if norm > 32.0 * self._calib_norm or norm < self._calib_norm / 64.0:
            self.loss_scale_exp, self._calib_norm = None, None
            return True
        return False

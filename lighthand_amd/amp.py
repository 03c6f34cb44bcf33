"""Dynamic loss scaling for 16-bit training inside the captured step (torch.amp.GradScaler semantics, decided on the device).

``torch.amp.GradScaler`` decides on the host (``found_inf.item()`` before ``optimizer.step()``); ``TrainStep`` replays the whole
iteration as one hipGraph with no host sync.  Here the decision lives in device memory and the step's last three launches make it
(``optim.Adam.step(amp=...)``, include/lighthand_hip.h):

* ``lh_amp_check``: is any element of the raw fp32 gradient arena inf / NaN (before unscaling, as
  ``torch._amp_foreach_non_finite_check_and_unscale_``: with a tiny scale a finite 1e38 gradient is not flagged);
* ``lh_amp_update``: ``found_inf``, ``inv = extra / scale``, the scale update of ``torch._amp_update_scale_`` and -- only for a
  finite step -- Adam's step counter / bias corrections;
* ``lh_adam_apply_guarded``: the Adam update with ``inv``, skipped whole when ``found_inf`` (params, moments, step unchanged, as
  when GradScaler skips ``optimizer.step()``).

The loss gradient of the next replay is formed with the updated ``scale`` (``lh_mse_heatmap`` reads it from the device).
"""
import torch

from . import _lib


class DynamicLossScale:
    """The device state of one dynamic loss scale.  Defaults and argument checks are those of ``torch.amp.GradScaler``.

    ``.scale`` / ``.skipped_steps`` read the device (one sync); ``.found_inf`` is the device int32 flag of the last step.
    ``state_dict()`` / ``load_state_dict()`` use GradScaler's keys, in both directions; loading writes the device tensors in
    place, so a step that has already captured its graph keeps training with the loaded state."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, device="cuda"):
        if not growth_factor > 1.0:
            raise AssertionError("The growth factor must be > 1.0.")
        if not backoff_factor < 1.0:
            raise AssertionError("The backoff factor must be < 1.0.")
        self.device = torch.device(device)
        self._scale = torch.full((1,), float(init_scale), dtype=torch.float32, device=self.device)
        self._growth_tracker = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._found_inf = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._skipped = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._inv = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._hyper = torch.zeros(3, dtype=torch.float64, device=self.device)       # growth, backoff, interval
        self._partial = torch.zeros(_lib.load().lh_amp_check_blocks(), dtype=torch.int32, device=self.device)   # per workgroup
        self._set_hyper(growth_factor, backoff_factor, growth_interval)

    def _set_hyper(self, growth_factor, backoff_factor, growth_interval):
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._hyper.copy_(torch.tensor([self.growth_factor, self.backoff_factor, float(self.growth_interval)], dtype=torch.float64))

    @property
    def scale(self):
        return float(self._scale.item())

    @property
    def found_inf(self):
        return self._found_inf

    @property
    def skipped_steps(self):
        return int(self._skipped.item())

    @property
    def scale_tensor(self):
        """The device fp32 [1] scale the loss gradient is multiplied by (read by lh_mse_heatmap at every replay)."""
        return self._scale

    def state_dict(self):
        return {"scale": self.scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(self._growth_tracker.item())}

    def load_state_dict(self, state_dict):
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._scale.fill_(float(state_dict["scale"]))
        self._growth_tracker.fill_(int(state_dict["_growth_tracker"]))
        self._set_hyper(state_dict["growth_factor"], state_dict["backoff_factor"], state_dict["growth_interval"])

    # -- TrainStep: the warm-up / capture iterations must not move the scale (nor count a growth tick or a skip)
    def _snapshot(self):
        return [t.clone() for t in (self._scale, self._growth_tracker, self._found_inf, self._skipped)]

    def _restore(self, snap):
        for t, s in zip((self._scale, self._growth_tracker, self._found_inf, self._skipped), snap):
            t.copy_(s)

    @torch.no_grad()
    def check_and_update(self, grad, numel, extra, hyper, step, derived, stream):
        """lh_amp_check over grad[0:numel] + lh_amp_update: found_inf, inv = extra / scale, the new scale, and the Adam tick of a
        finite step (hyper / step / derived: the optimizer's device state)."""
        lib = _lib.load()
        _lib.check(lib.lh_amp_check(grad, numel, self._partial.data_ptr(), stream), "lh_amp_check")
        _lib.check(lib.lh_amp_update(self._partial.data_ptr(), self._hyper.data_ptr(), self._scale.data_ptr(),
                                     self._growth_tracker.data_ptr(), self._found_inf.data_ptr(), self._skipped.data_ptr(),
                                     self._inv.data_ptr(), float(extra), hyper, step, derived, stream), "lh_amp_update")

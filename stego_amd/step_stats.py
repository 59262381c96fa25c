"""Step statistics that stay on the device (include/stego_stats.h): ``StepStats`` stands in for what the reference's ``training_step``
does for its TensorBoard log - three ``cd.mean()`` launches per step and, on histogram steps, three ``.cpu()`` copies with
``np.histogram`` over TensorBoard's default bins (train_segmentation.py:144-146, 165-177).

``record()`` is one kernel launch on torch's current stream: it reads up to four float32 tensors once and writes a fixed-size record -
counts, extremes, fp64 sum and sum of squares, the 1548 bucket counts when asked to, and up to 16 scalars copied from their device
addresses - into slot ``step % ring_slots`` of a ring in device memory.  The step counter lives on the device, so consecutive calls
have the same arguments and a call can be captured into a graph.  ``drain()`` is one device-to-host copy of the ring; between two
drains the host never waits for the GPU.

The record's layout is read from ``stego_step_stats_plan``; nothing here restates it.
"""
import warnings

import numpy as np
import torch

from . import capi


def _on_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("stego_amd runs on MI355X only: got a %s tensor (no CPU fallback exists)" % t.device)


def default_bins():
    """TensorBoard's default bucket limits (1549 float64), as the kernel's table holds them."""
    return capi.step_stats_edges()[0]


class StepStats:
    """``StepStats(n_scalars, ring_slots, device)`` owns the ring, the 16 bytes of state (step counter and ticket) and the workspace.
    Every ``record()`` of one object takes the same number of tensors (``n_tensors``, fixed by the first call unless given here)."""

    def __init__(self, n_scalars, ring_slots, device, n_tensors=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("stego_amd runs on MI355X only: StepStats on %s (no CPU fallback exists)" % device)
        if not 0 <= int(n_scalars) <= capi.STATS_MAX_SCALARS:
            raise ValueError("StepStats: %d scalars (0 .. %d)" % (n_scalars, capi.STATS_MAX_SCALARS))
        if not 1 <= int(ring_slots) <= capi.STATS_MAX_SLOTS:
            raise ValueError("StepStats: %d ring slots (1 .. %d)" % (ring_slots, capi.STATS_MAX_SLOTS))
        self.n_scalars, self.ring_slots, self.device = int(n_scalars), int(ring_slots), device
        self.n_tensors = None
        self.plan = None
        self.ring = None
        self._state = self._workspace = None
        self._drained = 0             # records [0, _drained) have been returned or given up
        self._warned = False
        if n_tensors is not None:
            self._allocate(int(n_tensors))

    def _allocate(self, n_tensors):
        rc, plan = capi.step_stats_plan(capi.stats_desc([0] * n_tensors, self.n_scalars, 0, self.ring_slots))
        if rc:
            raise ValueError("StepStats: %d tensors (1 .. %d)" % (n_tensors, capi.STATS_MAX_TENSORS))
        self.n_tensors, self.plan = n_tensors, plan
        self.ring = torch.zeros(plan["ring_bytes"], dtype=torch.uint8, device=self.device)
        self._state = torch.zeros(plan["state_bytes"] // 8, dtype=torch.int64, device=self.device)
        self._workspace = torch.zeros(plan["workspace_bytes"] // 8, dtype=torch.int64, device=self.device)
        self._desc = capi.stats_desc([0] * n_tensors, self.n_scalars, 0, self.ring_slots)
        self._tptr, self._sptr = capi.pointer_table(n_tensors), capi.pointer_table(self.n_scalars)
        self._addresses = (self.ring.data_ptr(), self._state.data_ptr(), self._workspace.data_ptr())

    def launch_plan(self, counts, with_hist=False):
        """The plan (grid, chunk, layout) of a record() over tensors of these counts."""
        rc, plan = capi.step_stats_plan(capi.stats_desc(counts, self.n_scalars, with_hist, self.ring_slots))
        if rc:
            raise RuntimeError("stego_step_stats_plan: error %d" % rc)
        return plan

    def record(self, tensors, scalars=(), with_hist=False):
        """One launch on the current stream: the statistics of `tensors` (1 .. 4 contiguous float32 tensors on the device; empty ones
        are allowed) and bit copies of `scalars` (n_scalars one-element float32 tensors or views) into the next slot of the ring."""
        if self.n_tensors is None:
            for t in tensors:
                _on_gpu(t)
            self._allocate(len(tensors))
        if len(tensors) != self.n_tensors or len(scalars) != self.n_scalars:
            raise ValueError("StepStats.record expects %d tensors and %d scalars, got %d and %d"
                             % (self.n_tensors, self.n_scalars, len(tensors), len(scalars)))
        # the descriptor and the two pointer tables are kept and filled in place: this runs once per training step
        desc, tptr, sptr = self._desc, self._tptr, self._sptr
        for i, t in enumerate(tensors):
            _on_gpu(t)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("StepStats.record expects contiguous float32 tensors, got %s %s" % (t.dtype, tuple(t.shape)))
            tptr[i] = t.data_ptr()
            desc.counts[i] = t.numel()
        for i, t in enumerate(scalars):
            _on_gpu(t)
            if t.dtype != torch.float32 or t.numel() != 1:
                raise ValueError("StepStats.record expects one-element float32 scalars, got %s %s" % (t.dtype, tuple(t.shape)))
            sptr[i] = t.data_ptr()
        desc.with_hist = 1 if with_hist else 0
        capi.step_stats_call(desc, tptr, sptr, self._addresses, self.device)

    def steps_recorded(self):
        """The device's step counter (a host read: it waits for the stream)."""
        return int(self._state[0])

    def drain(self):
        """One copy of the ring to the host -> the records newer than the last drain, in step order: dicts with `step`, `with_hist`,
        `scalars` (float32 [n_scalars]) and `tensors`, a list of dicts with n_finite, n_nan, n_out, min, max, sum, sum_sq, mean
        (sum / n_finite; nan without a finite value) and counts (uint32 [1548], or None for a record without buckets).  Records that
        were overwritten before they were drained are lost; that is said once, with a warning."""
        if self.ring is None:
            return []
        p = self.plan
        host = self.ring.cpu().numpy().reshape(self.ring_slots, p["record_bytes"])
        # the step of every slot; slots never written hold zeros and are told apart by their position
        found = {}
        for s in range(self.ring_slots):
            step = int(host[s, p["off_step"]:p["off_step"] + 8].view(np.int64)[0])
            n_t = int(host[s, p["off_n_tensors"]:p["off_n_tensors"] + 4].view(np.int32)[0])
            if n_t == self.n_tensors and step % self.ring_slots == s and step >= self._drained:
                found[step] = s
        if not found:
            return []
        newest = max(found)
        lost = (min(found) - self._drained) if newest - self._drained + 1 > self.ring_slots else 0
        if lost > 0 and not self._warned:
            self._warned = True
            warnings.warn("StepStats: %d records were overwritten before they were drained (ring_slots = %d): drain more often or "
                          "use a larger ring" % (lost, self.ring_slots))
        out = [self._parse(host[found[step]], step) for step in sorted(found)]
        self._drained = newest + 1
        return out

    def _parse(self, row, step):
        p = self.plan

        def field(off, dtype, n=1):
            return row[off:off + n * np.dtype(dtype).itemsize].view(dtype)

        with_hist = bool(field(p["off_with_hist"], np.int32)[0])
        tensors = []
        for i in range(self.n_tensors):
            base = p["off_tensors"] + i * p["tensor_stride"]
            n_finite = int(field(base + p["t_n_finite"], np.int64)[0])
            s = float(field(base + p["t_sum"], np.float64)[0])
            tensors.append(dict(
                n_finite=n_finite, n_nan=int(field(base + p["t_n_nan"], np.int64)[0]), n_out=int(field(base + p["t_n_out"], np.int64)[0]),
                min=np.float32(field(base + p["t_min"], np.float32)[0]), max=np.float32(field(base + p["t_max"], np.float32)[0]),
                sum=s, sum_sq=float(field(base + p["t_sum_sq"], np.float64)[0]), mean=s / n_finite if n_finite else float("nan"),
                counts=field(p["off_hist"] + i * p["hist_stride"], np.uint32, capi.STATS_BUCKETS).copy() if with_hist else None))
        return dict(step=step, with_hist=with_hist, scalars=field(p["off_scalars"], np.float32, self.n_scalars).copy(), tensors=tensors)

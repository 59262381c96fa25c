"""The parameter update of the training step as one native call (include/stego_optim.h): ``FusedAdam`` stands in for the three
``torch.optim.Adam`` of ``LitUnsupervisedSegmenter.configure_optimizers`` (train_segmentation.py:117-119, 228-230 of the reference).

One object owns what the three optimizers own between them - the flat ``exp_avg`` / ``exp_avg_sq`` buffers, one step counter per group
on the device, the segment table - and reads gradients from one flat bucket (``ddp.FlatGradReducer``: the model's under data
parallelism, otherwise one of its own), which the kernel zeroes as it goes.  ``groups[i]`` are facades with the optimizer protocol the
trainer and the checkpoints use; their ``state_dict()`` has exactly the layout of ``torch.optim.Adam.state_dict()`` for the same
parameter list, so checkpoints written with and without ``cfg.native_optim`` load into each other.

One difference from torch: a trainable parameter that received no gradient has a zero gradient in the bucket, not ``None``, and takes
a momentum-only step (the data-parallel path behaves this way with torch's optimizers too).

Construction, ``state_dict``, ``load_state_dict`` and ``reset_group`` work on any device; ``step()`` needs a HIP device.
"""
import torch

from . import capi, ddp


class _Group:
    """One logical optimizer of a FusedAdam with the slice of the torch.optim.Optimizer protocol the trainer uses."""

    def __init__(self, owner, index, params, lr, betas, eps):
        self._owner, self._index = owner, index
        # a torch Adam that never steps: it holds param_groups (this torch's hyperparameter keys and defaults, the saved indices of
        # state_dict) and validates what load_state_dict is given the way torch does
        self._template = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
        self.params = list(self._template.param_groups[0]["params"])
        self.trainable = [(i, p) for i, p in enumerate(self.params) if p.requires_grad]
        self.param_groups = self._template.param_groups

    def hyper(self):
        """(lr, beta1, beta2, eps) as they stand now; refuses what the kernel does not compute."""
        g = self.param_groups[0]
        _plain_adam(g)
        return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])

    def step(self):
        """This group alone, in one launch (the trainer steps all groups at once: FusedAdam.step)."""
        self._owner.step(only=self._index)

    def zero_grad(self, set_to_none=False):
        """Zeroes this group's slices of the bucket; the .grad views stay (set_to_none would detach them and is ignored)."""
        self._owner._zero_group_grads(self._index)

    def state_dict(self):
        return self._owner._group_state_dict(self._index)

    def load_state_dict(self, sd):
        self._owner._load_group_state_dict(self._index, sd)


def _plain_adam(g):
    if g.get("amsgrad", False) or g.get("maximize", False) or g.get("weight_decay", 0) != 0:
        raise ValueError("FusedAdam is plain Adam: amsgrad=%r, maximize=%r, weight_decay=%r are not supported"
                         % (g.get("amsgrad", False), g.get("maximize", False), g.get("weight_decay", 0)))
    if len(g["betas"]) != 2 or any(torch.is_tensor(x) for x in (g["lr"], g["eps"]) + tuple(g["betas"])):
        raise ValueError("FusedAdam takes lr, betas and eps as Python numbers")


class FusedAdam:
    """``FusedAdam(groups)``: ``groups`` is a list of ``{"params": [...], "lr": ..., "betas": ..., "eps": ...}`` (the last three
    optional, torch's defaults).  Frozen parameters may be handed over, as ``self.net.parameters()`` does: they keep their index in
    ``state_dict()`` and are never touched.  ``reducer``: the ``FlatGradReducer`` whose bucket holds the gradients (it must cover
    every trainable parameter of the groups); without one the optimizer builds its own, and ``.grad`` of every trainable parameter
    becomes a view into it."""

    def __init__(self, groups, reducer=None, zero_grads=True):
        if not 1 <= len(groups) <= capi.ADAM_MAX_GROUPS:
            raise ValueError("FusedAdam: %d groups (1 .. %d)" % (len(groups), capi.ADAM_MAX_GROUPS))
        self.zero_grads = bool(zero_grads)
        self.bucket_zeroed = False        # True after a step of every group that zeroed the gradients it read
        self.groups = []
        for i, g in enumerate(groups):
            g = dict(g)
            _plain_adam({"betas": (0, 0), "lr": 0, "eps": 0, **g})
            unknown = set(g) - {"params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"}
            if unknown:
                raise ValueError("FusedAdam: unknown group keys %s" % sorted(unknown))
            params = list(g["params"])
            for p in params:
                if p.requires_grad and p.dtype != torch.float32:
                    raise ValueError("FusedAdam expects float32 parameters, got %s" % p.dtype)
            self.groups.append(_Group(self, i, params, g.get("lr", 1e-3), tuple(g.get("betas", (0.9, 0.999))), g.get("eps", 1e-8)))
        trainable = [p for grp in self.groups for _, p in grp.trainable]
        if not trainable:
            raise ValueError("FusedAdam: no trainable parameters")
        if len({id(p) for p in trainable}) != len(trainable):
            raise ValueError("FusedAdam: a parameter appears in more than one group")
        if len(trainable) > capi.ADAM_MAX_SEGMENTS:
            raise ValueError("FusedAdam: %d trainable tensors (at most %d)" % (len(trainable), capi.ADAM_MAX_SEGMENTS))
        self.device = trainable[0].device
        if any(p.device != self.device for p in trainable):
            raise ValueError("FusedAdam expects its parameters on one device")
        self.numel = sum(p.numel() for p in trainable)
        if self.numel >= capi.ADAM_MAX_ELEMS:
            raise ValueError("FusedAdam: %d elements (fewer than 2^31)" % self.numel)
        # state slices: group after group, tensor after tensor, each padded to a multiple of 4 floats so that the two moments are
        # 16-byte aligned wherever the parameter is
        self._state_off, off = {}, 0
        self._state_range = []
        for grp in self.groups:
            begin = off
            for _, p in grp.trainable:
                self._state_off[id(p)] = off
                off += (p.numel() + 3) // 4 * 4
            self._state_range.append((begin, off))
        self.exp_avg = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros(off, dtype=torch.float32, device=self.device)
        self._counters = torch.zeros(capi.ADAM_MAX_GROUPS + 1, dtype=torch.int32, device=self.device)
        self.steps = self._counters[:len(self.groups)]          # one per group, advanced by the kernel
        self._ticket = self._counters[capi.ADAM_MAX_GROUPS:]    # the kernel's last-workgroup ticket: zero between calls
        self.bucket = None
        self.use_bucket(reducer if reducer is not None else ddp.FlatGradReducer(trainable))

    # ---- the gradient bucket and the segment table
    def use_bucket(self, reducer):
        """Read gradients from `reducer`'s flat buffer from now on (the model's bucket when data parallelism sets one up later)."""
        at, off = {}, 0
        for p in reducer.params:
            at[id(p)] = off
            off += p.numel()
        records = []
        for gi, grp in enumerate(self.groups):
            for _, p in grp.trainable:
                if id(p) not in at:
                    raise ValueError("FusedAdam: the gradient bucket does not hold a trainable parameter of group %d" % gi)
                if not p.is_contiguous():
                    raise ValueError("FusedAdam expects contiguous parameters")
                records.append((p.data_ptr(), p.numel(), at[id(p)], self._state_off[id(p)], gi))
        if reducer.flat.device != self.device:
            raise ValueError("FusedAdam: the gradient bucket is on %s, the parameters on %s" % (reducer.flat.device, self.device))
        self.bucket = reducer
        self._records = records
        self._table_host = capi.adam_segments(records)
        raw = torch.frombuffer(bytearray(bytes(self._table_host)), dtype=torch.uint8)
        self._table = raw.to(self.device) if self.device.type != "cpu" else raw.clone()
        self._grad_ranges = []
        for gi in range(len(self.groups)):
            spans = sorted((r[2], r[2] + r[1]) for r in records if r[4] == gi)
            merged = []
            for a, b in spans:
                if merged and merged[-1][1] == a:
                    merged[-1][1] = b
                else:
                    merged.append([a, b])
            self._grad_ranges.append(merged)
        # what the bucket holds beyond the groups (a trainable tensor that no optimizer owns): the kernel never zeroes it
        self._uncovered, at_end = [], 0
        for a, b in sorted((r[2], r[2] + r[1]) for r in records) + [(off, off)]:
            if a > at_end:
                self._uncovered.append((at_end, a))
            at_end = max(at_end, b)

    def _zero_group_grads(self, gi):
        for a, b in self._grad_ranges[gi]:
            self.bucket.flat[a:b].zero_()

    def zero_uncovered(self):
        """Zeroes the slices of the bucket that belong to no group (none when the optimizer built its own bucket): with the fused
        zeroing on, this is all that is left of the start-of-step zero_grad."""
        for a, b in self._uncovered:
            self.bucket.flat[a:b].zero_()

    def zero_grad(self):
        """The whole bucket in one launch (what the trainer does when the fused zeroing is off); the .grad views stay."""
        self.bucket.zero_grad()

    def plan(self):
        """(grid, chunk, n_chunks) of the launch step() makes."""
        rc, grid, chunk, n = capi.adam_plan(self._desc(None), self._table_host)
        if rc:
            raise RuntimeError("stego_adam_plan: error %d" % rc)
        return grid, chunk, n

    def _desc(self, only):
        hyper = [grp.hyper() + (1 if only is None or only == i else 0,) for i, grp in enumerate(self.groups)]
        return capi.adam_desc(len(self._records), hyper, self.zero_grads, self.bucket.flat.numel(), self.exp_avg.numel())

    def step(self, only=None):
        """One Adam step of every group (or of group `only`) in one kernel launch on the current stream: lr, betas and eps are read
        from the groups now, the step counters stay on the device, and nothing synchronises with the host."""
        if self._records[0][0] != self.groups[self._records[0][4]].trainable[0][1].data_ptr():
            self.use_bucket(self.bucket)        # the parameters moved (module.to(), load with assign=True): new addresses
        capi.adam_step(self._desc(only), self._table_host, self._table, self.bucket.flat, self.exp_avg, self.exp_avg_sq, self.steps,
                       self._ticket)
        self.bucket_zeroed = self.zero_grads and only is None

    def reset_group(self, gi):
        """Group gi as a freshly built optimizer: moments and step counter zero (the probe reset of train_segmentation.py:373-383)."""
        a, b = self._state_range[gi]
        self.exp_avg[a:b].zero_()
        self.exp_avg_sq[a:b].zero_()
        self.steps[gi:gi + 1].zero_()

    # ---- checkpoints in torch.optim.Adam's layout
    def _group_state_dict(self, gi):
        grp = self.groups[gi]
        sd = grp._template.state_dict()           # param_groups with indices; the template's own state is empty
        t = int(self.steps[gi])
        state = {}
        if t > 0:                                 # a fresh torch Adam has no state either
            for i, p in grp.trainable:
                a = self._state_off[id(p)]
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32),
                            "exp_avg": self.exp_avg[a:a + p.numel()].view_as(p).clone(),
                            "exp_avg_sq": self.exp_avg_sq[a:a + p.numel()].view_as(p).clone()}
        sd["state"] = state
        return sd

    def _load_group_state_dict(self, gi, sd):
        grp = self.groups[gi]
        if len(sd["param_groups"]) != 1:
            raise ValueError("FusedAdam group %d: expected one param group, got %d" % (gi, len(sd["param_groups"])))
        _plain_adam(sd["param_groups"][0])
        index = {i: p for i, p in grp.trainable}
        state = sd.get("state", {})
        steps = set()
        for k, st in state.items():
            if k not in index:
                raise ValueError("FusedAdam group %d: state for parameter %r, which is not a trainable parameter of the group" % (gi, k))
            if "max_exp_avg_sq" in st:
                raise ValueError("FusedAdam is plain Adam: the state holds amsgrad's max_exp_avg_sq")
            p = index[k]
            if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError("FusedAdam group %d: state of parameter %r has shape %s, the parameter %s"
                                 % (gi, k, tuple(st["exp_avg"].shape), tuple(p.shape)))
            steps.add(float(st["step"]))
        if len(steps) > 1 or (state and len(state) != len(index)):
            raise ValueError("FusedAdam group %d keeps one step counter: the state holds steps %s over %d of %d trainable parameters"
                             % (gi, sorted(steps), len(state), len(index)))
        t = steps.pop() if steps else 0.0
        if t != int(t) or not 0 <= t < 2 ** 31:
            raise ValueError("FusedAdam group %d: step %r is not a count" % (gi, t))
        # hyperparameters and the group's size, checked and taken over by torch itself
        grp._template.load_state_dict({"state": {}, "param_groups": sd["param_groups"]})
        grp.param_groups = grp._template.param_groups
        self.reset_group(gi)
        for k, st in state.items():
            p = index[k]
            a = self._state_off[id(p)]
            self.exp_avg[a:a + p.numel()].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[a:a + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))
        self.steps[gi:gi + 1].fill_(int(t))

    def state_dict(self):
        return [grp.state_dict() for grp in self.groups]

    def load_state_dict(self, sds):
        if len(sds) != len(self.groups):
            raise ValueError("FusedAdam: %d state dicts for %d groups" % (len(sds), len(self.groups)))
        for grp, sd in zip(self.groups, sds):
            grp.load_state_dict(sd)

"""The fused Adam step without a GPU: every host check of stego_adam_step (include/stego_optim.h) returns its documented code before
anything is launched, stego_adam_plan covers every element of a ragged segment list exactly once, FusedAdam's state dicts are
torch.optim.Adam's key for key and value for value in both directions, what one step counter cannot hold is refused, reset_group
resets one group, and checkpoints written with cfg.native_optim off and on load into each other."""
import math
import warnings

import pytest
import torch

from stego_amd import capi
from stego_amd.optim import FusedAdam

warnings.filterwarnings("ignore", message="DinoFeaturizer")

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read
NULL, ALIGN = 1, 5   # STEGO_ERR_NULL, STEGO_ERR_ALIGN
GROUP = (5e-4, 0.9, 0.999, 1e-8)


def _table(records=None):
    return capi.adam_segments(records if records is not None else [(A, 70, 0, 0, 0), (A + 0x1000, 1917, 70, 72, 1), (A + 0x9000, 5, 1987, 1992, 2)])


def _desc(n_segments=3, groups=None, zero=1, grad_elems=4096, state_elems=4096, n_groups=None):
    return capi.adam_desc(n_segments, groups if groups is not None else [GROUP] * 3, zero, grad_elems, state_elems, n_groups=n_groups)


def _rc(desc=None, table=None, segs=A, grads=A, m=A, v=A, steps=A, ticket=A, **kw):
    return capi.adam_step_raw(desc if desc is not None else _desc(**kw), table if table is not None else _table(), segs, grads, m, v,
                              steps, ticket)


def test_a_valid_call_passes_every_check_up_to_the_last():
    """The stand-in call is valid but for one misaligned pointer, the last thing checked: nothing is launched."""
    assert _rc(ticket=A + 2) == ALIGN
    assert capi.adam_plan(_desc(), _table())[0] == 0


@pytest.mark.parametrize("which", ["desc", "table", "segs", "grads", "m", "v", "steps", "ticket", "param"])
def test_null_pointers(which):
    if which == "desc":
        assert capi.adam_step_raw(None, _table(), A, A, A, A, A, A) == NULL
        assert capi.adam_plan(None, _table())[0] == NULL
    elif which == "table":
        assert capi.adam_step_raw(_desc(), None, A, A, A, A, A, A) == NULL
        assert capi.adam_plan(_desc(), None)[0] == NULL
    elif which == "param":
        t = _table([(A, 70, 0, 0, 0), (None, 8, 70, 72, 1), (A, 5, 80, 80, 2)])
        assert _rc(table=t) == NULL and capi.adam_plan(_desc(), t)[0] == NULL
    else:
        assert _rc(**{which: None}) == NULL


@pytest.mark.parametrize("kw,rc", [
    (dict(n_segments=0), capi.OPTIM_ERR_COUNT), (dict(n_segments=-1), capi.OPTIM_ERR_COUNT), (dict(n_segments=257), capi.OPTIM_ERR_COUNT),
    (dict(n_groups=0), capi.OPTIM_ERR_COUNT), (dict(n_groups=9), capi.OPTIM_ERR_COUNT),
    (dict(zero=2), capi.OPTIM_ERR_FLAGS), (dict(zero=-1), capi.OPTIM_ERR_FLAGS),
    (dict(groups=[GROUP + (0,)] * 3), capi.OPTIM_ERR_FLAGS), (dict(groups=[GROUP, GROUP + (2,), GROUP]), capi.OPTIM_ERR_FLAGS),
    (dict(groups=[GROUP, (5e-3, 1.0, 0.999, 1e-8), GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[GROUP, (5e-3, 0.9, 1.0, 1e-8), GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[GROUP, (5e-3, -0.1, 0.999, 1e-8), GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[GROUP, (5e-3, 0.9, math.nan, 1e-8), GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[GROUP, GROUP, (5e-3, 0.9, 0.999, -1e-8)]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[GROUP, GROUP, (5e-3, 0.9, 0.999, math.inf)]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[(math.nan, 0.9, 0.999, 1e-8), GROUP, GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[(-1e-3, 0.9, 0.999, 1e-8), GROUP, GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(groups=[(math.inf, 0.9, 0.999, 1e-8), GROUP, GROUP]), capi.OPTIM_ERR_PARAM),
    (dict(n_groups=2), capi.OPTIM_ERR_SEGMENT),                    # the third segment's group index 2 is out of range
    (dict(grad_elems=1991), capi.OPTIM_ERR_SEGMENT), (dict(state_elems=1996), capi.OPTIM_ERR_SEGMENT),
])
def test_descriptor_checks(kw, rc):
    assert _rc(**kw) == rc
    assert capi.adam_plan(_desc(**kw), _table()) == (rc, 0, 0, 0)


def test_an_inactive_group_is_not_validated_and_the_limits_are_inclusive():
    bad = (math.nan, 1.0, 1.0, -1.0, 0)
    assert _rc(groups=[GROUP, bad, GROUP], ticket=A + 2) == ALIGN
    assert _rc(groups=[(0.0, 0.0, 0.0, 0.0)] * 3, ticket=A + 2) == ALIGN              # lr, betas and eps of 0 are values, not errors
    assert _rc(grad_elems=1992, state_elems=1997, ticket=A + 2) == ALIGN              # slices that end where their buffer ends


@pytest.mark.parametrize("rec,rc", [
    ((A, 0, 0, 0, 0), capi.OPTIM_ERR_SEGMENT), ((A, -5, 0, 0, 0), capi.OPTIM_ERR_SEGMENT),
    ((A, 8, 0, 0, 3), capi.OPTIM_ERR_SEGMENT), ((A, 8, 0, 0, -1), capi.OPTIM_ERR_SEGMENT),
    ((A, 8, -1, 0, 0), capi.OPTIM_ERR_SEGMENT), ((A, 8, 0, -4, 0), capi.OPTIM_ERR_SEGMENT),
    ((A, 8, 4089, 0, 0), capi.OPTIM_ERR_SEGMENT), ((A, 8, 0, 4089, 0), capi.OPTIM_ERR_SEGMENT),
    ((A, 1 << 31, 0, 0, 0), capi.OPTIM_ERR_COUNT),
])
def test_segment_checks(rec, rc):
    t = _table([(A, 70, 0, 0, 0), rec, (A, 5, 1987, 1992, 2)])
    assert _rc(table=t) == rc
    assert capi.adam_plan(_desc(), t)[0] == rc


def test_total_elements_stay_below_2_to_31():
    big = 1 << 40
    t = _table([(A, (1 << 30), 0, 0, 0), (A, (1 << 30), 0, 0, 1)])
    assert _rc(desc=_desc(2, grad_elems=big, state_elems=big), table=t) == capi.OPTIM_ERR_COUNT
    t = _table([(A, (1 << 30), 0, 0, 0), (A, (1 << 30) - 1, 0, 0, 1)])
    assert _rc(desc=_desc(2, grad_elems=big, state_elems=big), table=t, ticket=A + 2) == ALIGN
    rc, grid, chunk, n = capi.adam_plan(_desc(2, grad_elems=big, state_elems=big), t)
    assert (rc, grid, chunk, n) == (0, capi.ADAM_MAX_GRID, capi.ADAM_CHUNK, 2 * (1 << 20))


@pytest.mark.parametrize("which", ["segs", "grads", "m", "v", "steps", "ticket", "param"])
def test_misaligned_pointers(which):
    if which == "param":
        for off in (1, 2, 3):
            assert _rc(table=_table([(A, 70, 0, 0, 0), (A + off, 8, 70, 72, 1), (A, 5, 80, 80, 2)])) == ALIGN
        assert _rc(table=_table([(A, 70, 0, 0, 0), (A + 4, 8, 70, 72, 1), (A, 5, 80, 80, 2)]), ticket=A + 2) == ALIGN   # 4 bytes are enough
        return
    assert _rc(**{which: A + 2}) == ALIGN
    if which == "segs":
        assert _rc(segs=A + 4) == ALIGN                              # the table holds pointers and int64: 8-byte alignment
    else:
        assert _rc(**{which: A + 4, "segs": A + 4}) == ALIGN         # float32 / int32: 4 bytes are enough; fails on the next thing wrong


def test_error_strings():
    lib = capi.load()
    for rc in (capi.OPTIM_ERR_COUNT, capi.OPTIM_ERR_SEGMENT, capi.OPTIM_ERR_PARAM, capi.OPTIM_ERR_FLAGS):
        assert lib.stego_error_string(rc).decode().startswith("fused Adam:"), rc
    for name in ("stego_adam_step", "stego_adam_plan"):
        assert hasattr(lib, name) and name in capi.SIGNATURES


def test_plan_covers_a_ragged_segment_list_exactly_once():
    counts = [1, 3, 4, 5, 70, 1917, 1024, 1025, 2048, 5000, 1023]
    records, off = [], 0
    for i, n in enumerate(counts):
        records.append((A, n, off, off, i % 3))
        off += n
    rc, grid, chunk, n_chunks = capi.adam_plan(_desc(len(counts), grad_elems=off, state_elems=off), _table(records))
    assert rc == 0 and chunk == capi.ADAM_CHUNK and n_chunks == sum(-(-n // chunk) for n in counts) and grid == n_chunks
    seen = torch.zeros(off, dtype=torch.int32)
    taken = []
    for b in range(grid):                                            # workgroup b takes chunks b, b + grid, ...
        taken += list(range(b, n_chunks, grid))
    assert sorted(taken) == list(range(n_chunks))
    for c in taken:                                                  # the header's rule, restated
        first = 0
        for (_, n, goff, _, _) in records:
            nc = -(-n // chunk)
            if c < first + nc:
                lo, hi = (c - first) * chunk, min(n, (c - first + 1) * chunk)
                assert lo < hi
                seen[goff + lo:goff + hi] += 1
                break
            first += nc
        else:
            raise AssertionError("chunk %d belongs to no segment" % c)
    assert bool((seen == 1).all())


# ---- FusedAdam on the CPU: the state dicts of torch.optim.Adam
def _tiny_model(**kw):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=32", "batch_size=2", "dim=12"] + ["%s=%s" % (k, v) for k, v in kw.items()]
    torch.manual_seed(1)
    return LitUnsupervisedSegmenter(5, load_config(overrides=ov)).cpu()


def _stepped_adams(model, steps=2, seed=0):
    """The reference's three optimizers after `steps` steps on seeded gradients."""
    g = torch.Generator().manual_seed(seed)
    adams = list(model.configure_optimizers())
    for _ in range(steps):
        for o in adams:
            for p in o.param_groups[0]["params"]:
                if p.requires_grad:
                    p.grad = torch.randn(p.shape, generator=g) * 1e-2
            o.step()
    return adams


def _same(a, b, path="state_dict"):
    assert type(a) is type(b) or (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), (path, list(a.keys()), list(b.keys()))
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    else:
        assert a == b, (path, a, b)


def test_state_dict_interchange_with_torch_adam():
    model = _tiny_model()
    groups = model.optimizer_groups()
    frozen = [p for p in groups[0]["params"] if not p.requires_grad]
    assert frozen and any(p.requires_grad for p in groups[0]["params"])        # group 0 carries the frozen backbone's parameters
    adams = _stepped_adams(model)
    fused = FusedAdam(groups)
    for facade, adam in zip(fused.groups, adams):
        assert facade.state_dict()["state"] == {}                             # never stepped: no state, as a fresh torch Adam
        _same(facade.state_dict()["param_groups"], adam.state_dict()["param_groups"])
        want = adam.state_dict()
        facade.load_state_dict(want)
        got = facade.state_dict()
        _same(got, want)
        assert sorted(got["state"]) == [i for i, p in enumerate(adam.param_groups[0]["params"]) if p.requires_grad]
        assert all(float(s["step"]) == 2.0 for s in got["state"].values())
        fresh = torch.optim.Adam(adam.param_groups[0]["params"], lr=123.0)
        fresh.load_state_dict(got)
        _same(fresh.state_dict(), want)
    assert fused.steps.tolist() == [2, 2, 2]
    assert len(fused.groups[0].state_dict()["param_groups"][0]["params"]) == len(groups[0]["params"])
    for p in fused.bucket.params:                                              # every trainable .grad is a view into the bucket
        assert p.grad.data_ptr() >= fused.bucket.flat.data_ptr() and p.grad.shape == p.shape
    # hyperparameters come from the loaded dict, as with torch
    sd = adams[1].state_dict()
    sd["param_groups"][0]["lr"] = 0.25
    fused.groups[1].load_state_dict(sd)
    assert fused.groups[1].param_groups[0]["lr"] == 0.25 and fused.groups[1].hyper()[0] == 0.25


def test_what_one_counter_cannot_hold_is_refused():
    model = _tiny_model()
    adams = _stepped_adams(model)
    fused = FusedAdam(model.optimizer_groups())
    sd = adams[1].state_dict()
    keys = sorted(sd["state"])
    assert len(keys) == 2
    sd["state"][keys[1]]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="one step counter"):
        fused.groups[1].load_state_dict(sd)
    sd = adams[1].state_dict()
    del sd["state"][keys[1]]                                                    # one parameter stepped, the other never
    with pytest.raises(ValueError, match="one step counter"):
        fused.groups[1].load_state_dict(sd)
    params = list(model.linear_probe.parameters())
    for kw in (dict(amsgrad=True), dict(weight_decay=0.1), dict(maximize=True)):
        other = torch.optim.Adam(params, lr=5e-3, **kw)
        for p in params:
            p.grad = torch.ones_like(p)
        other.step()
        with pytest.raises(ValueError, match="plain Adam"):
            fused.groups[1].load_state_dict(other.state_dict())
        with pytest.raises(ValueError, match="plain Adam"):
            FusedAdam([{"params": params, "lr": 5e-3, **kw}])
    assert fused.steps.tolist() == [0, 0, 0]                                    # a refused load changes nothing
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))]}])
    with pytest.raises(ValueError, match="more than one group"):
        FusedAdam([{"params": params}, {"params": params[:1]}])
    with pytest.raises(ValueError, match="no trainable"):
        FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(3), requires_grad=False)]}])


def test_reset_group_zeroes_one_group_and_leaves_the_others():
    model = _tiny_model()
    adams = _stepped_adams(model)
    fused = FusedAdam(model.optimizer_groups())
    fused.load_state_dict([o.state_dict() for o in adams])
    before = [f.state_dict() for f in fused.groups]
    fused.reset_group(1)
    assert fused.steps.tolist() == [2, 0, 2]
    assert fused.groups[1].state_dict()["state"] == {}
    a, b = fused._state_range[1]
    assert not fused.exp_avg[a:b].any() and not fused.exp_avg_sq[a:b].any()
    _same(fused.groups[0].state_dict(), before[0])
    _same(fused.groups[2].state_dict(), before[2])


def test_a_shared_bucket_may_hold_more_than_the_groups():
    """Under data parallelism the model's bucket covers every trainable tensor, also those no optimizer owns: the table points into
    it, and what the kernel will not zero is known."""
    from stego_amd import ddp
    a, b, c, d = (torch.nn.Parameter(torch.zeros(n)) for n in (5, 70, 3, 9))
    reducer = ddp.FlatGradReducer([a, b, c, d])
    fused = FusedAdam([{"params": [b]}, {"params": [d]}], reducer=reducer)
    assert fused.bucket is reducer and [(r[1], r[2], r[4]) for r in fused._records] == [(70, 5, 0), (9, 78, 1)]
    assert fused._uncovered == [(0, 5), (75, 78)]
    reducer.flat.fill_(1.0)
    fused.zero_uncovered()
    assert reducer.flat.tolist() == [0.0] * 5 + [1.0] * 70 + [0.0] * 3 + [1.0] * 9
    fused.groups[1].zero_grad()
    assert reducer.flat.tolist() == [0.0] * 5 + [1.0] * 70 + [0.0] * 12
    own = FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(6))]}])
    assert own._uncovered == []
    with pytest.raises(ValueError, match="does not hold"):
        FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(2))]}], reducer=reducer)
    later = ddp.FlatGradReducer([d, c, b])                               # setup_distributed() after the optimizers were built
    fused.use_bucket(later)
    assert [(r[1], r[2]) for r in fused._records] == [(70, 12), (9, 0)] and fused._uncovered == [(9, 12)]


def test_step_needs_a_hip_device():
    fused = FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(5))]}])
    with pytest.raises(RuntimeError, match="MI355X only"):
        fused.step()
    assert fused.plan() == (1, capi.ADAM_CHUNK, 1)


def test_checkpoints_load_across_the_flag(tmp_path):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    assert load_config().native_optim is False and load_config().native_optim_zero is True
    model = _tiny_model()
    assert model.cfg.native_optim is False
    model._optims = _stepped_adams(model)
    path = str(tmp_path / "off.ckpt")
    model.save_checkpoint(path)
    want = [o.state_dict() for o in model._optims]
    on = LitUnsupervisedSegmenter.load_from_checkpoint(path, native_optim=True)
    assert on.cfg.native_optim is True
    for o, w in zip(on.optimizers(), want):                          # a CPU model keeps torch's optimizers, whatever the flag says
        assert isinstance(o, torch.optim.Adam)
        _same(o.state_dict(), w)
    # what the trainer does once the model is on its device: the facades take the loaded state over ...
    fused = FusedAdam(on.optimizer_groups())
    fused.load_state_dict([o.state_dict() for o in on.optimizers()])
    for f, w in zip(fused.groups, want):
        _same(f.state_dict(), w)
    # ... and a checkpoint written from them loads with the flag off
    on._fused, on._optims = fused, list(fused.groups)
    path2 = str(tmp_path / "on.ckpt")
    on.save_checkpoint(path2)
    off = LitUnsupervisedSegmenter.load_from_checkpoint(path2, native_optim=False)
    for o, w in zip(off.optimizers(), want):
        assert isinstance(o, torch.optim.Adam)
        _same(o.state_dict(), w)

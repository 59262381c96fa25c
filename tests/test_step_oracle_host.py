"""tests/step_oracle.py, the float64 yardstick of tests/test_all_native_step_gpu.py, against torch autograd on the CPU: a
LitUnsupervisedSegmenter with every extension key off and native_backbone=False, cast to .double(), runs two training_steps on the
shape and the inputs of the GPU test; every logged loss/* term, the gradient of every trainable parameter and the parameters after the
update must agree with the composition.  The correspondence term has no torch chain in the product: it goes through the oracle-backed
backend double of tests/oracle_backend.py, here with its outputs left in the dtype of its inputs (it casts to float32 for the device
tests) and the step's weight vector in float64, so that the comparison is float64 against float64 end to end.  No GPU."""
import warnings

import numpy as np
import pytest
import torch

import aug_oracle
import oracle_backend
import step_oracle as SO
from stego_amd import modules as M
from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config

RTOL = 1e-9                 # of the largest element: float64 sums of a few thousand terms in two orders


@pytest.mark.parametrize("proj", ["nonlinear", "linear"])
def test_the_composition_is_the_double_precision_training_step(monkeypatch, proj):
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=SO.SHAPE + SO.WEIGHTS + ["native_backbone=False", "projection_type=%s" % proj])
    for key in ("native_probes", "native_crf_loss", "native_rec_loss", "native_aug", "native_optim", "train_log", "cache_backbone_tokens"):
        assert getattr(cfg, key) is False, key
    torch.manual_seed(1)                    # (the seed of the GPU test)
    model = LitUnsupervisedSegmenter(SO.N_CLASSES, cfg).cpu().double()
    model.net.dropout.p = 0.0
    names = SO.trainable_names(model)
    assert ("net.cluster2.0.weight" in names) == (proj == "nonlinear") and "decoder.weight" in names and len(names) == (11 if proj == "nonlinear" else 7)
    named = dict(model.named_parameters())
    monkeypatch.setattr(oracle_backend, "_t", lambda a, like: torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype))
    loss_fn = model.contrastive_corr_loss_fn
    weights = (cfg.pos_intra_weight, cfg.pos_inter_weight, cfg.neg_inter_weight)
    loss_fn._weights = {(tuple(float(w) for w in weights), torch.device("cpu")): torch.tensor(weights, dtype=torch.float64)}
    kept, hook = SO.capture_feats(model)
    ds = SyntheticContrastiveDataset(4 * SO.B, SO.RES, SO.N_CLASSES)
    monkeypatch.setattr(M, "_backend", oracle_backend)
    try:
        for step in range(2):
            batch = SO.step_batch(ds, step)
            coords1, coords2, perms, points, table = SO.step_draws(step)
            img_aug, coord_aug = aug_oracle.augment(batch["img"], table, SO.RES, torch.float64)
            batch = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
            batch["img_aug"], batch["coord_aug"] = img_aug, coord_aug
            SO.feed_draws(model, coords1, coords2, perms, points)
            before = {n: named[n].detach().clone() for n in names}
            adam = {id(p): s for o in model.optimizers() for p, s in o.state.items()}
            state = {n: (adam[id(named[n])]["exp_avg"].clone(), adam[id(named[n])]["exp_avg_sq"].clone()) if id(named[n]) in adam else None
                     for n in names}
            del kept[:]
            loss = model.training_step(batch, step)
            assert len(kept) == 3 and all(t.dtype == torch.float64 for t in kept)
            ref = SO.step_oracle(cfg, before, kept[0], kept[1], kept[2], batch["img"], batch["label"], coord_aug, coords1, coords2, perms, points)
            assert ref["gap"] >= SO.MIN_GAP, ref["gap"]
            tags = sorted(k for k in model.logged if k.startswith("loss/"))
            assert tags == sorted(ref["losses"]) and len(tags) == 9, tags
            for k in tags:
                got, want = float(model.logged[k]), ref["losses"][k]
                print("step %d %s: torch %.15g oracle %.15g" % (step, k, got, want))
                assert abs(got - want) <= 1e-11 * max(1.0, abs(want)), k
            assert abs(loss.item() - ref["losses"]["loss/total"]) <= 1e-11
            for k in ("cd/pos_intra", "cd/pos_inter", "cd/neg_inter"):
                assert abs(float(model.logged[k]) - ref["cd"][k]) <= 1e-11, k
            if proj == "nonlinear":
                assert ref["ambiguous"].dtype == torch.bool and tuple(ref["ambiguous"].shape) == (192,)
            lrs = {n: g["lr"] for g in model.optimizer_groups() for p in g["params"] for n in names if named[n] is p}
            for n in names:
                got, want = named[n].grad.detach(), ref["grads"][n]
                assert got.shape == want.shape, n
                scale = float(want.abs().max())
                err = float((got - want).abs().max())
                print("step %d %s: max|g| %.3e max|torch - oracle| %.3e" % (step, n, scale, err))
                assert scale > 0 and err <= RTOL * scale, (n, err, scale)
                m, v = state[n] if state[n] is not None else (torch.zeros_like(before[n]), torch.zeros_like(before[n]))
                after = SO.adam_update64(before[n], got, lrs[n], step, m, v)
                assert np.abs(named[n].detach().numpy().reshape(-1) - after).max() <= 1e-12, n         # torch's Adam in double is adam64
    finally:
        hook.remove()
    assert oracle_backend.calls.count("corr_fwd") >= 2            # the correspondence term did go through the double

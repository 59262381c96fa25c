"""The directory dataset on the MI355X: stego_data_prepare_dir (DeviceImageStore.from_directory) against the CPU DirectoryDataset
transform bit for bit - with labels, without, and from a store reduced with store_res - DeviceContrastiveLoader on such a store
against the CPU ContrastiveSegDataset("directory"), and precompute -> train -> eval on a small folder, labelled and unlabelled."""
import math
import os
import shutil
from os.path import join

import numpy as np
import pytest
import torch

from directory_folder import bits, files, open_pair, restated_item, write_folder
from stego_amd import data as D
from stego_amd import device_data as DD
from stego_amd.precompute_knns import nns_filename, save_nns

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAME = "photos"
# (h, w): 1 x 500 and 500 x 1, a short side equal to each tested R, tiny upscales, sizes around the tile of 16 pixels per lane
SIZES = [(1, 500), (500, 1), (224, 300), (400, 224), (6, 9), (11, 6), (37, 50), (64, 37), (3, 2), (1, 1), (7, 6), (2, 3),
         (40, 52), (36, 30), (225, 223), (230, 340), (100, 100), (65, 63), (38, 36), (17, 5), (129, 257), (240, 320), (320, 240),
         (48, 64), (5, 5), (90, 41), (33, 77), (250, 226), (12, 200), (150, 9)]
RES = [6, 37, 224]         # 6 and 37: one pixel per lane (R % 4 != 0, below and above 64 pixels per row of lanes); 224: 16 per lane


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """The labelled folder (image 3 is the grey file, image 4 the RGBA one) and a copy of it without `labels`."""
    root = tmp_path_factory.mktemp("dirs")
    write_folder(root, NAME, "train", SIZES, seed=5, grey=3, rgba=4)
    bare = tmp_path_factory.mktemp("dirs_bare")
    shutil.copytree(join(str(root), NAME, "imgs"), join(str(bare), NAME, "imgs"))
    return str(root), str(bare)


_REFS = {}


def _refs(root, R, origins=None):
    """The restated items of the folder at R, computed once per (folder, R, centre | origins) and shared by the cases."""
    key = (root, R, origins is not None)
    if key not in _REFS:
        imgs, labs = files(root, NAME, "train")
        _REFS[key] = [restated_item(*open_pair(imgs, labs, i), R, None if origins is None else tuple(int(v) for v in origins[i]))
                      for i in range(len(imgs))]
    return _REFS[key]


def _origins(R):
    rng = np.random.default_rng(R)
    span = np.array([(nh - R, nw - R) for nw, nh in (D.resized_size(w, h, R) for h, w in reversed(SIZES))])     # sorted order = reversed
    return np.stack([rng.integers(0, span[:, 0] + 1), rng.integers(0, span[:, 1] + 1)], 1).astype(np.int32)


@pytest.mark.parametrize("variant", ["labels", "no_labels", "store_res"])
@pytest.mark.parametrize("R", RES)
def test_prepare_dir_is_bitwise_the_cpu_directory_transform(folders, R, variant):
    root = folders[1] if variant == "no_labels" else folders[0]
    store = DD.DeviceImageStore.from_directory(root, NAME, "train", device=DEV, store_res=R if variant == "store_res" else None)
    n = len(SIZES)
    assert len(store) == n and store.kind == "directory" and (store.labels is None) == (variant == "no_labels")
    if variant == "store_res":
        assert store.nbytes == DD.directory_bytes(root, NAME, "train", store_res=R) < DD.directory_bytes(root, NAME, "train")
    ind = torch.arange(n, dtype=torch.int64, device=DEV)
    org = _origins(R)
    for origin in (None, org):
        o = None if origin is None else torch.from_numpy(origin).to(DEV)
        img, label, mask = store.prepare(ind, R, o, validate=True)
        again = store.prepare(ind, R, o)
        torch.cuda.synchronize()
        assert img.dtype == torch.float32 and label.dtype == torch.int64 and mask.dtype == torch.float32
        assert tuple(img.shape) == (n, 3, R, R) and tuple(label.shape) == (n, R, R) and tuple(mask.shape) == (n, 1, R, R)
        for a, b in zip((img, label, mask), again):             # deterministic
            assert torch.equal(bits(a), bits(b))
        img, label, mask = img.cpu(), label.cpu(), mask.cpu()
        saw = set()
        for i, (ref_img, ref_label, ref_mask) in enumerate(_refs(root, R, origin)):
            assert torch.equal(bits(img[i]), bits(ref_img)), (i, R, variant)
            assert torch.equal(label[i], ref_label), (i, R, variant)
            assert torch.equal(bits(mask[i]), bits(ref_mask)), (i, R, variant)
            saw.update(np.unique(ref_label.numpy()).tolist())
        assert saw == {-1} if variant == "no_labels" else {0, 1, 255} <= saw and -1 not in saw
    # a permuted, repeated index list lands in the order asked for
    perm = torch.tensor([n - 1, 0, 7, 7, 3], dtype=torch.int64, device=DEV)
    img, label, mask = store.prepare(perm, R)
    refs = _refs(root, R)
    for j, i in enumerate(perm.tolist()):
        assert torch.equal(bits(img[j].cpu()), bits(refs[i][0])) and torch.equal(label[j].cpu(), refs[i][1])


def test_a_reduced_store_refuses_another_resolution(folders):
    store = DD.DeviceImageStore.from_directory(folders[0], NAME, "train", device=DEV, store_res=224)
    ind = torch.arange(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="store_res = 224 and serves that resolution only, not R = 320"):
        store.prepare(ind, 320)
    assert tuple(store.prepare(ind, 224)[2].shape) == (2, 1, 224, 224)


def _random_nns(n, k=10, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([[i], rng.permutation(np.delete(np.arange(n), i))[:k - 1]]) for i in range(n)]).astype(np.int64)


@pytest.mark.parametrize("crop", ["center", "random"])
def test_loader_on_a_directory_store_matches_the_cpu_dataset(folders, tmp_path, crop):
    root = folders[0]
    n, R, B, K, world = len(SIZES), 16, 4, 5, 2
    nns = _random_nns(n)
    store = DD.DeviceImageStore.from_directory(root, NAME, "train", device=DEV)
    imgs, labs = files(root, NAME, "train")
    cpu = {i: open_pair(imgs, labs, i) for i in range(n)}
    # the CPU dataset gives the same items for the same index (centre crops: no draw takes part)
    os.makedirs(join(str(tmp_path), "nns"))
    save_nns(join(str(tmp_path), "nns", nns_filename("vit_small", NAME, "train", None, R)), nns)
    os.symlink(join(root, NAME), join(str(tmp_path), NAME))
    import types
    cfg = types.SimpleNamespace(crop_ratio=0.5, model_type="vit_small", res=R, dir_dataset_name=NAME, dir_dataset_n_classes=5)
    ds = D.ContrastiveSegDataset(str(tmp_path), "directory", None, "train", D.image_transform(R), D.label_transform(R), cfg,
                                 num_neighbors=K, mask=True, pos_images=True, pos_labels=True)
    for rank in range(world):
        loader = DD.DeviceContrastiveLoader(store, nns, B, K, R, crop=crop, seed=3, rank=rank, world=world, aug=(rank == 1))
        assert len(loader) == math.ceil(n / world) // B and loader.dataset.n_cache_items == n
        for epoch in range(2):
            seen = []
            for b in loader:
                keys = {"ind", "img", "label", "mask", "img_pos", "ind_pos", "label_pos", "mask_pos"}
                assert set(b) == (keys | {"img_aug", "coord_aug"} if rank == 1 else keys)
                assert all(v.device.type == "cuda" for v in b.values())
                assert b["mask"].dtype == torch.float32 and tuple(b["mask"].shape) == (B, 1, R, R) and tuple(b["label"].shape) == (B, R, R)
                if rank == 1:
                    assert tuple(b["img_aug"].shape) == (B, 3, R, R) and bool(torch.isfinite(b["img_aug"]).all())
                ind, ind_pos = b["ind"].cpu().numpy(), b["ind_pos"].cpu().numpy()
                org = loader.last_origin.cpu().numpy() if crop == "random" else None
                for j in range(len(ind)):
                    assert ind_pos[j] in nns[ind[j], 1:K + 1]
                    for which, idx, o in (("", ind[j], j), ("_pos", ind_pos[j], len(ind) + j)):
                        rgb, lab = cpu[int(idx)]
                        ref = restated_item(rgb, lab, R, None if crop == "center" else (int(org[o, 0]), int(org[o, 1])))
                        assert torch.equal(bits(b["img" + which][j].cpu()), bits(ref[0]))
                        assert torch.equal(b["label" + which][j].cpu(), ref[1])
                        assert torch.equal(bits(b["mask" + which][j].cpu()), bits(ref[2]))
                    if crop == "center":
                        it = ds[int(ind[j])]
                        assert torch.equal(bits(it["img"]), bits(b["img"][j].cpu())) and torch.equal(it["label"], b["label"][j].cpu())
                        assert torch.equal(bits(it["mask"]), bits(b["mask"][j].cpu()))
                seen += ind.tolist()
            order = DD.epoch_indices(n, world, rank, 3, epoch).tolist()
            assert seen == order[:len(loader) * B] and len(set(seen)) == len(seen)


# ---- precompute -> train -> eval on a folder of 24 training images and 8 for validation
TINY = ["model_type=vit_tiny", "dino_patch_size=16", "batch_size=4", "num_workers=0", "dim=16", "max_steps=3", "val_freq=2",
        "scalar_log_freq=1", "pretrained_weights=~", "dataset_name=directory", "dir_dataset_name=%s" % NAME, "dir_dataset_n_classes=5",
        "res=64"]


def _chain_folder(root, name, split, n, seed):
    """n images of about 72 x 96 with labels 0 .. 4 (mode-L PNGs), in DirectoryDataset's layout."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for kind in ("imgs", "labels"):
        os.makedirs(join(str(root), name, kind, split), exist_ok=True)
    for i in range(n):
        h, w = 72 + 4 * (i % 3), 96 + 2 * (i % 5)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(join(str(root), name, "imgs", split, "p%03d.jpg" % i))
        Image.fromarray(rng.integers(0, 5, (h, w)).astype(np.uint8), "L").save(join(str(root), name, "labels", split, "p%03d.png" % i))


@pytest.fixture(scope="module")
def chain_roots(tmp_path_factory):
    root = tmp_path_factory.mktemp("chain")
    _chain_folder(root, NAME, "train", 24, 21)
    _chain_folder(root, NAME, "val", 8, 22)
    bare = tmp_path_factory.mktemp("chain_bare")
    shutil.copytree(join(str(root), NAME, "imgs", "train"), join(str(bare), NAME, "imgs", "train"))
    return str(root), str(bare)


def test_precompute_train_and_eval_on_a_labelled_folder(chain_roots, capsys):
    from stego_amd import eval_segmentation, precompute_knns, train_segmentation
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    root = chain_roots[0]
    ov = TINY + ["pytorch_data_dir=%s" % root, "output_root=%s" % root]
    written = precompute_knns.my_app(load_config(overrides=ov))
    names = ["nns_vit_tiny_%s_%s_None_224.npz" % (NAME, s) for s in ("val", "train")]
    assert [os.path.basename(p) for p in written] == names
    for s, name in zip(("val", "train"), names):
        nns = np.load(join(root, "nns", name))["nns"]
        n = 8 if s == "val" else 24
        assert nns.shape == (n, n) and nns.dtype == np.int64            # fewer than 30 images: every other image is a neighbour
        assert all(sorted(row) == list(range(n)) for row in nns.tolist())
        assert (nns[:, 0] == np.arange(len(nns))).mean() > 0.9
    assert precompute_knns.my_app(load_config(overrides=ov)) == []       # both exist: skipped
    # training reads the table of cfg.res, as the reference's dataset does: the same neighbours under that name
    shutil.copy(join(root, "nns", names[1]), join(root, "nns", "nns_vit_tiny_%s_train_None_64.npz" % NAME))
    capsys.readouterr()

    cfg = load_config(overrides=ov + ["experiment_name=full"])
    losses = train_segmentation.my_app(cfg)
    out = capsys.readouterr().out
    assert "training data: device store of the folder at full size (24 images" in out
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    ckpt = train_segmentation.checkpoint_path(cfg)
    model = LitUnsupervisedSegmenter.load_from_checkpoint(ckpt)
    assert model.global_step == 3 and model.n_classes == 5

    # over the budget at full size (24 images of about 72 x 96 x 4 bytes), inside it reduced to 64: the store_res path, and it says so
    full, small = DD.directory_bytes(root, NAME, "train"), DD.directory_bytes(root, NAME, "train", store_res=64)
    assert small < full
    cfg2 = load_config(overrides=ov + ["experiment_name=reduced", "device_dataset_max_gb=%r" % ((small + 1) / 2 ** 30), "val_freq=100"])
    losses2 = train_segmentation.my_app(cfg2)
    out = capsys.readouterr().out
    assert "training data: device store reduced to store_res = 64 (24 images" in out and "budget is" in out
    assert len(losses2) == 3 and all(math.isfinite(v) for v in losses2)

    ecfg = load_config(eval_segmentation.EVAL_CONFIG, overrides=["pytorch_data_dir=%s" % root, "model_paths=[%s]" % ckpt, "res=64",
                                                                  "batch_size=8", "run_crf=True"])
    metrics = eval_segmentation.my_app(ecfg)[ckpt]
    assert "synthetic" not in capsys.readouterr().out
    assert {"final/linear/mIoU", "final/cluster/mIoU", "final/linear/Accuracy", "final/cluster/Accuracy"} <= set(metrics)
    assert all(math.isfinite(float(v)) for v in metrics.values())


@pytest.mark.parametrize("native_probes", [False, True])
def test_an_unlabelled_folder_trains_with_a_nan_linear_loss_and_finite_gradients(chain_roots, capsys, monkeypatch, native_probes):
    from stego_amd import train_segmentation
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    root = chain_roots[1]
    os.makedirs(join(root, "nns"), exist_ok=True)
    save_nns(join(root, "nns", "nns_vit_tiny_%s_train_None_64.npz" % NAME), _random_nns(24, 30))
    logged = []
    log = LitUnsupervisedSegmenter.log

    def record(self, name, value, **kw):
        logged.append((name, value.detach().clone() if torch.is_tensor(value) else value))
        return log(self, name, value, **kw)
    monkeypatch.setattr(LitUnsupervisedSegmenter, "log", record)
    cfg = load_config(overrides=TINY + ["pytorch_data_dir=%s" % root, "output_root=%s" % root, "native_probes=%s" % native_probes,
                                        "experiment_name=bare%d" % native_probes])
    losses = train_segmentation.my_app(cfg)
    out = capsys.readouterr().out
    assert "has no labels folder" in out and "loss/linear and loss/total are NaN" in out
    assert "no labelled val split in the folder: training without validation" in out
    assert len(losses) == 3 and all(math.isnan(v) for v in losses)
    by_name = {}
    for name, value in logged:
        by_name.setdefault(name, []).append(float(value))
    assert len(by_name["loss/linear"]) == 3 and all(math.isnan(v) for v in by_name["loss/linear"] + by_name["loss/total"])
    for name in ("loss/cluster", "loss/pos_intra", "loss/pos_inter", "loss/neg_inter"):
        assert len(by_name[name]) == 3 and all(math.isfinite(v) for v in by_name[name]), name
    model = LitUnsupervisedSegmenter.load_from_checkpoint(train_segmentation.checkpoint_path(cfg))
    assert model.global_step == 3
    for name, p in model.state_dict().items():
        assert bool(torch.isfinite(p.float()).all()), name

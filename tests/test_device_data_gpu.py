"""The device-resident dataset on the MI355X: stego_data_prepare against the CPU transforms bit for bit, DeviceContrastiveLoader
against the CPU ContrastiveSegDataset, the descriptor errors, and the precompute -> train -> eval chain on a small cropped tree."""
import math
import os
from os.path import join

import numpy as np
import pytest
import torch
from PIL import Image

from stego_amd import capi
from stego_amd import data as D
from stego_amd import device_data as DD
from stego_amd.precompute_knns import nns_filename, save_nns

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _write_split(root, split, imgs, labels):
    d = D.crop_dir(str(root), "cocostuff27", "five", 0.5)
    os.makedirs(join(d, "img", split), exist_ok=True)
    os.makedirs(join(d, "label", split), exist_ok=True)
    for i, (im, lb) in enumerate(zip(imgs, labels)):
        im.save(join(d, "img", split, "%d.jpg" % i), "JPEG")
        Image.fromarray(lb, "L").save(join(d, "label", split, "%d.png" % i), "PNG")
    return d


def _open(d, split, i):
    with Image.open(join(d, "img", split, "%d.jpg" % i)) as im:
        rgb = im.convert("RGB")
    with Image.open(join(d, "label", split, "%d.png" % i)) as lb:
        lab = lb.copy()
    return rgb, lab


def _at_origin(rgb, lab, R, top, left):
    """Resize-then-crop at an explicit origin, with image_transform's arithmetic."""
    box = (left, top, left + R, top + R)
    x = np.asarray(D._resize(rgb, R).crop(box), dtype=np.float32) / np.float32(255.0)
    img = torch.from_numpy(((x - D._MEAN) / D._STD).transpose(2, 0, 1).copy())
    return img, torch.as_tensor(np.array(D._resize(lab, R).crop(box)), dtype=torch.int64) - 1


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def sizes_tree(tmp_path_factory):
    """230 crops of 220+ distinct sizes: random sizes, 1 x 500, 500 x 1, short side = 224 and = 320, tiny upscales, a greyscale JPEG,
    label bytes 0 and 255."""
    root = tmp_path_factory.mktemp("sizes")
    rng = np.random.default_rng(7)
    shapes = [(1, 500), (500, 1), (224, 300), (400, 224), (320, 333), (321, 320), (6, 9), (3, 2), (1, 1), (7, 6)]
    shapes += [tuple(int(v) for v in rng.integers(1, 420, 2)) for _ in range(220)]
    imgs, labels = [], []
    for k, (h, w) in enumerate(shapes):
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        imgs.append(Image.fromarray(arr[..., 0], "L") if k == 3 else Image.fromarray(arr, "RGB"))
        lab = rng.integers(0, 28, (h, w)).astype(np.uint8)
        lab[rng.random((h, w)) < 0.05] = 255
        labels.append(lab)
    d = _write_split(root, "train", imgs, labels)
    return root, d, len(shapes)


@pytest.mark.parametrize("R", [6, 224, 320])
def test_prepare_is_bitwise_the_cpu_transform(sizes_tree, R):
    root, d, n = sizes_tree
    store = DD.DeviceImageStore(str(root), "cocostuff27", "five", 0.5, "train", device=DEV)
    assert len(store) == n
    ind = torch.arange(n, dtype=torch.int64, device=DEV)
    img, label, mask = store.prepare(ind, R)
    again = store.prepare(ind, R)
    torch.cuda.synchronize()
    assert img.dtype == torch.float32 and label.dtype == torch.int64 and mask.dtype == torch.bool
    assert tuple(img.shape) == (n, 3, R, R) and tuple(label.shape) == (n, R, R) and tuple(mask.shape) == (n, 1, R, R)
    for a, b in zip((img, label, mask), again):                 # deterministic
        assert torch.equal(_bits(a), _bits(b))
    img, label, mask = img.cpu(), label.cpu(), mask.cpu()
    saw = set()
    for i in range(n):
        rgb, lab = _open(d, "train", i)
        ref_img = D.image_transform(R)(rgb)
        ref_lab = D.label_transform(R)(lab)[0] - 1
        assert torch.equal(_bits(img[i]), _bits(ref_img)), (i, rgb.size, R)
        assert torch.equal(label[i], ref_lab), (i, rgb.size, R)
        assert torch.equal(mask[i, 0], ref_lab == -1)
        saw.update(np.unique(ref_lab.numpy()).tolist())
    assert -1 in saw and 254 in saw                               # stored 0 and 255

    # explicit origins: uniform over the resized image
    rec = store.table(R)["records"]
    rng = np.random.default_rng(R)
    org = np.stack([rng.integers(0, rec["nh"] - R + 1), rng.integers(0, rec["nw"] - R + 1)], 1).astype(np.int32)
    perm = rng.permutation(n)
    img, label, mask = (t.cpu() for t in store.prepare(torch.from_numpy(perm).to(DEV), R, torch.from_numpy(org[perm]).to(DEV),
                                                        validate=True))
    for j, i in enumerate(perm[:80]):
        rgb, lab = _open(d, "train", int(i))
        ref_img, ref_lab = _at_origin(rgb, lab, R, int(org[i, 0]), int(org[i, 1]))
        assert torch.equal(_bits(img[j]), _bits(ref_img)), (i, rgb.size, R, org[i])
        assert torch.equal(label[j], ref_lab) and torch.equal(mask[j, 0], ref_lab == -1)


def test_invalid_requests_are_rejected_before_a_launch(sizes_tree):
    root, _, n = sizes_tree
    store = DD.DeviceImageStore(str(root), "cocostuff27", "five", 0.5, "train", device=DEV)
    t = store.table(8)
    ind = torch.arange(4, dtype=torch.int64, device=DEV)
    img = torch.full((4, 3, 8, 8), 7.0, device=DEV)
    label = torch.full((4, 8, 8), 7, dtype=torch.int64, device=DEV)
    mask = torch.ones(4, 1, 8, 8, dtype=torch.bool, device=DEV)
    R_, n_items, ib, lb, ml = t["desc"]
    for desc, code in [(capi.data_desc(4, 0, n_items, ib, lb, ml), capi.DATA_ERR_RES),
                       (capi.data_desc(0, 8, n_items, ib, lb, ml), capi.DATA_ERR_COUNT),
                       (capi.data_desc(4, 8, 0, ib, lb, ml), capi.DATA_ERR_COUNT)]:
        rc = capi.data_prepare_raw(desc, t["items"], store.images, store.labels, t["maps"], store.lut, ind, None, img, label, mask)
        assert rc == code
    rc = capi.data_prepare_raw(capi.data_desc(4, 8, n_items, ib, lb, ml), t["items"], store.images, store.labels, t["maps"], store.lut,
                               ind, None, img[:, :, :, 1:], label, mask)
    assert rc == 5                                                    # misaligned output: STEGO_ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((img == 7).all()) and bool((label == 7).all()) and bool(mask.all())       # nothing ran
    with pytest.raises(ValueError, match="index %d at position 1 outside" % n):
        store.prepare(torch.tensor([0, n], device=DEV), 8, validate=True)
    with pytest.raises(ValueError, match="does not fit R = 8"):
        store.prepare(torch.tensor([0], device=DEV), 8, torch.tensor([[0, 10 ** 6]], dtype=torch.int32, device=DEV), validate=True)
    with pytest.raises(ValueError, match="outside"):
        store.prepare(ind, capi.DATA_MAX_RES + 1)


def _small_tree(root, n_src, split, seed, hw=(64, 48)):
    g = torch.Generator().manual_seed(seed)
    items = [(torch.rand(3, hw[0] + 4 * (i % 3), hw[1] + 2 * (i % 5), generator=g), torch.randint(-1, 27, (hw[0] + 4 * (i % 3), hw[1] + 2 * (i % 5)), generator=g))
             for i in range(n_src)]
    return D.write_cropped(str(root), "cocostuff27", "five", 0.5, split, items)


def _random_nns(n, k=10, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([[i], rng.permutation(np.delete(np.arange(n), i))[:k - 1]]) for i in range(n)]).astype(np.int64)


def _batches(loader, epochs):
    out = []
    for _ in range(epochs):
        out.append([{k: v.clone() for k, v in b.items()} for b in loader])
    return out


@pytest.mark.parametrize("crop", ["center", "random"])
def test_loader_matches_the_cpu_dataset_and_visits_every_index(tmp_path, crop):
    n = _small_tree(tmp_path, 10, "train", 0)
    nns = _random_nns(n)
    R, B, K, world = 16, 4, 5, 2
    store = DD.DeviceImageStore(str(tmp_path), "cocostuff27", "five", 0.5, "train", device=DEV)
    d = D.crop_dir(str(tmp_path), "cocostuff27", "five", 0.5)
    cpu = {i: _open(d, "train", i) for i in range(n)}
    for rank in range(world):
        loader = DD.DeviceContrastiveLoader(store, nns, B, K, R, crop=crop, seed=3, rank=rank, world=world)
        twin = DD.DeviceContrastiveLoader(store, nns, B, K, R, crop=crop, seed=3, rank=rank, world=world)
        assert len(loader) == math.ceil(n / world) // B and loader.dataset.n_cache_items == n and loader.dataset.per_rank
        assert loader.dataset.deterministic_items == (crop == "center") and len(loader.dataset) == n
        for epoch in range(2):
            seen = []
            for b in loader:
                assert set(b) == {"ind", "img", "label", "mask", "img_pos", "ind_pos", "label_pos", "mask_pos"}
                assert all(v.device.type == "cuda" for v in b.values())
                ind, ind_pos = b["ind"].cpu().numpy(), b["ind_pos"].cpu().numpy()
                org = loader.last_origin.cpu().numpy() if crop == "random" else None
                for j in range(len(ind)):
                    assert ind_pos[j] in nns[ind[j], 1:K + 1]
                    for which, idx, o in (("", ind[j], j), ("_pos", ind_pos[j], len(ind) + j)):
                        rgb, lab = cpu[int(idx)]
                        if crop == "center":
                            ref_img, ref_lab = D.image_transform(R)(rgb), D.label_transform(R)(lab)[0] - 1
                        else:
                            ref_img, ref_lab = _at_origin(rgb, lab, R, int(org[o, 0]), int(org[o, 1]))
                        assert torch.equal(_bits(b["img" + which][j].cpu()), _bits(ref_img))
                        assert torch.equal(b["label" + which][j].cpu(), ref_lab)
                        assert torch.equal(b["mask" + which][j, 0].cpu(), ref_lab == -1)
                seen += ind.tolist()
            order = DD.epoch_indices(n, world, rank, 3, epoch).tolist()
            assert seen == order[:len(loader) * B] and len(set(seen)) == len(seen)
        a, b2 = _batches(twin, 2), _batches(DD.DeviceContrastiveLoader(store, nns, B, K, R, crop=crop, seed=3, rank=rank, world=world), 2)
        for ea, eb in zip(a, b2):
            for x, y in zip(ea, eb):
                assert all(torch.equal(_bits(x[k]), _bits(y[k])) for k in x)


def test_sequential_mode_covers_the_split_in_order(tmp_path):
    n = _small_tree(tmp_path, 3, "val", 1)
    store = DD.DeviceImageStore(str(tmp_path), "cocostuff27", "five", 0.5, "val", device=DEV)
    loader = DD.DeviceContrastiveLoader(store, None, batch_size=4, res=12, drop_last=False)
    batches = list(loader)
    assert len(loader) == len(batches) == math.ceil(n / 4)
    assert set(batches[0]) == {"img", "label", "mask", "ind"}
    assert torch.cat([b["ind"] for b in batches]).tolist() == list(range(n))
    assert tuple(batches[-1]["img"].shape) == (n - 4 * (len(batches) - 1), 3, 12, 12)


# ---- precompute -> train -> eval on a tree of 40 source images (200 training crops) and 8 for validation (40 crops)
TINY = ["model_type=vit_tiny", "dino_patch_size=16", "batch_size=4", "num_workers=0", "dim=16", "max_steps=3", "val_freq=2",
        "scalar_log_freq=1", "pretrained_weights=~"]


@pytest.fixture(scope="module")
def real_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tree")
    assert _small_tree(root, 40, "train", 11, hw=(72, 96)) == 200
    assert _small_tree(root, 8, "val", 12, hw=(72, 96)) == 40
    return root


def test_precompute_train_and_eval_on_a_cropped_tree(real_tree, capsys):
    from stego_amd import eval_segmentation, precompute_knns, train_segmentation
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    root = str(real_tree)
    ov = TINY + ["pytorch_data_dir=%s" % root, "output_root=%s" % root]
    written = precompute_knns.my_app(load_config(overrides=ov))
    names = [nns_filename("vit_tiny", "cocostuff27", s, "five", 224) for s in ("val", "train")]
    assert [os.path.basename(p) for p in written] == names
    for s, name in zip(("val", "train"), names):
        nns = np.load(join(root, "nns", name))["nns"]
        assert nns.shape == ((40 if s == "val" else 200), 30) and nns.dtype == np.int64
        assert (nns[:, 0] == np.arange(len(nns))).mean() > 0.9          # a crop is its own nearest neighbour (up to exact ties)
    assert precompute_knns.my_app(load_config(overrides=ov)) == []       # both exist: skipped

    for cache in (False, True):
        cfg = load_config(overrides=ov + ["cache_backbone_tokens=%s" % cache, "experiment_name=cache%d" % cache])
        losses = train_segmentation.my_app(cfg)
        out = capsys.readouterr().out
        assert "training data: device store (200 crops" in out
        assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
        ckpt = train_segmentation.checkpoint_path(cfg)
        model = LitUnsupervisedSegmenter.load_from_checkpoint(ckpt)
        assert model.global_step == 3 and model.n_classes == 27
    ecfg = load_config(eval_segmentation.EVAL_CONFIG, overrides=["pytorch_data_dir=%s" % root, "model_paths=[%s]" % ckpt, "res=64",
                                                                  "batch_size=8", "run_crf=True"])
    metrics = eval_segmentation.my_app(ecfg)[ckpt]
    assert {"final/linear/mIoU", "final/cluster/mIoU", "final/linear/Accuracy", "final/cluster/Accuracy"} <= set(metrics)
    assert all(math.isfinite(float(v)) for v in metrics.values())


def test_over_budget_store_falls_back_to_the_cpu_loader(real_tree, capsys):
    from stego_amd import train_segmentation
    from stego_amd.train_segmentation import load_config
    root = str(real_tree)
    with pytest.raises(DD.StoreTooLarge, match="budget is"):
        DD.DeviceImageStore(root, "cocostuff27", "five", 0.5, "train", device=DEV, max_bytes=1000)
    nns_dir = join(root, "nns")
    if not os.path.exists(join(nns_dir, nns_filename("vit_tiny", "cocostuff27", "train", "five", 224))):
        os.makedirs(nns_dir, exist_ok=True)
        save_nns(join(nns_dir, nns_filename("vit_tiny", "cocostuff27", "train", "five", 224)), _random_nns(200, 30))
    cfg = load_config(overrides=TINY + ["pytorch_data_dir=%s" % root, "output_root=%s" % root, "device_dataset_max_gb=1e-6",
                                        "experiment_name=cpu", "val_freq=100"])
    losses = train_segmentation.my_app(cfg)
    out = capsys.readouterr().out
    assert "training data: CPU loader (ContrastiveSegDataset, 0 workers)" in out and "budget is" in out
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)

"""Host side of the directory dataset (data.DirectoryDataset, ContrastiveSegDataset("directory"), DeviceImageStore.from_directory's
sizing and store_res claim, the host checks of stego_data_prepare_dir and stego_salience_coords).  No GPU needed."""
import ctypes
import os
import random
import shutil
import types
from os.path import join

import numpy as np
import pytest
import torch
from PIL import Image

from directory_folder import HOST_SIZES, bits, files, open_pair, restated_item, write_folder
from stego_amd import data as D
from stego_amd import device_data as DD
from stego_amd.precompute_knns import nns_filename, save_nns

NAME = "myphotos"


def _cfg(root, res=8, n_classes=5):
    return types.SimpleNamespace(crop_ratio=0.5, model_type="vit_small", res=res, pytorch_data_dir=str(root), dir_dataset_name=NAME,
                                 dir_dataset_n_classes=n_classes)


def _nns(root, n, res, k=4, seed=1):
    rng = np.random.default_rng(seed)
    nns = np.stack([np.concatenate([[i], rng.permutation(np.delete(np.arange(n), i))[:k - 1]]) for i in range(n)]).astype(np.int64)
    os.makedirs(join(str(root), "nns"), exist_ok=True)
    path = join(str(root), "nns", "nns_vit_small_%s_train_None_%d.npz" % (NAME, res))
    save_nns(path, nns)
    return nns, path


@pytest.mark.parametrize("R", [6, 224])
def test_directory_items_are_the_restated_transform_in_sorted_order(tmp_path, R):
    stems = write_folder(tmp_path, NAME, "train", HOST_SIZES)
    imgs, labs = files(tmp_path, NAME, "train")
    assert [os.path.basename(f).split(".")[0] for f in imgs] == stems and stems[0] == "im_0000"      # written last, listed first
    with Image.open(imgs[len(imgs) - 1 - 1]) as im:
        assert im.mode == "L"                                   # the grey file is image k = 1
    with Image.open(imgs[len(imgs) - 1 - 2]) as im:
        assert im.mode == "RGBA"
    ds = D.DirectoryDataset(str(tmp_path), NAME, "train", D.image_transform(R), D.label_transform(R))
    assert len(ds) == len(HOST_SIZES)
    seen = set()
    for i in range(len(ds)):
        img, label, mask = ds[i]
        ref_img, ref_label, ref_mask = restated_item(*open_pair(imgs, labs, i), R)
        assert img.dtype == torch.float32 and tuple(img.shape) == (3, R, R)
        assert label.dtype == torch.int64 and tuple(label.shape) == (R, R)
        assert mask.dtype == torch.float32 and tuple(mask.shape) == (1, R, R)
        assert torch.equal(bits(img), bits(ref_img)) and torch.equal(label, ref_label) and torch.equal(mask, ref_mask)
        assert torch.equal(mask[0], (label > 0).float())
        seen.update(np.unique(label.numpy()).tolist())
    assert {0, 1, 255} <= seen and -1 not in seen             # the stored value itself: no "- 1"


def test_random_crops_of_image_and_label_share_one_numpy_drawn_seed(tmp_path):
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    imgs, labs = files(tmp_path, NAME, "train")
    R = 6
    ds = D.DirectoryDataset(str(tmp_path), NAME, "train", D.image_transform(R, "random"), D.label_transform(R, "random"))
    for i in range(len(ds)):
        np.random.seed(40 + i)
        img, label, mask = ds[i]
        np.random.seed(40 + i)
        seed = int(np.random.randint(2147483647))
        rgb, lab = open_pair(imgs, labs, i)
        random.seed(seed)
        torch.manual_seed(seed)
        ref_img = D.image_transform(R, "random")(rgb)
        random.seed(seed)
        torch.manual_seed(seed)
        ref_label = D.label_transform(R, "random")(lab)[0]
        assert torch.equal(bits(img), bits(ref_img)) and torch.equal(label, ref_label)


def test_folder_without_labels_gives_minus_one_and_an_empty_mask(tmp_path):
    write_folder(tmp_path, NAME, "train", HOST_SIZES, labels=False)
    imgs, labs = files(tmp_path, NAME, "train")
    assert labs is None
    ds = D.DirectoryDataset(str(tmp_path), NAME, "train", D.image_transform(6), D.label_transform(6))
    for i in range(len(ds)):
        img, label, mask = ds[i]
        assert torch.equal(bits(img), bits(restated_item(*open_pair(imgs, labs, i), 6)[0]))
        assert label.dtype == torch.int64 and tuple(label.shape) == (6, 6) and bool((label == -1).all())
        assert mask.dtype == torch.float32 and tuple(mask.shape) == (1, 6, 6) and bool((mask == 0).all())


def test_mismatched_counts_an_empty_split_and_a_16_bit_label_raise(tmp_path):
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    imgs, labs = files(tmp_path, NAME, "train")
    os.makedirs(join(str(tmp_path), NAME, "imgs", "val"))
    os.makedirs(join(str(tmp_path), NAME, "labels", "val"))
    with pytest.raises(ValueError, match="empty split 'val'"):
        D.DirectoryDataset(str(tmp_path), NAME, "val", D.image_transform(6), D.label_transform(6))
    with pytest.raises(ValueError, match="empty split 'val'"):
        DD.directory_bytes(str(tmp_path), NAME, "val")
    Image.fromarray(np.full((5, 5), 300, dtype=np.uint16)).save(labs[1])          # a 16-bit PNG in place of an 8-bit one
    ds = D.DirectoryDataset(str(tmp_path), NAME, "train", D.image_transform(6), D.label_transform(6))
    ds[0]
    with pytest.raises(ValueError, match=os.path.basename(labs[1]).replace(".", r"\.")):
        ds[1]
    with pytest.raises(ValueError, match=os.path.basename(labs[1]).replace(".", r"\.")):
        DD.DeviceImageStore.from_directory(str(tmp_path), NAME, "train", device="cpu")
    os.remove(labs[0])
    with pytest.raises(AssertionError, match="4 images but 3 labels"):
        D.DirectoryDataset(str(tmp_path), NAME, "train", D.image_transform(6), D.label_transform(6))


def test_contrastive_directory_dataset_keys_shapes_positives_and_table_name(tmp_path):
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    n, R, K = len(HOST_SIZES), 224, 3
    path = join(str(tmp_path), "nns", nns_filename("vit_small", NAME, "train", None, R))
    assert os.path.basename(path) == "nns_vit_small_%s_train_None_224.npz" % NAME
    with pytest.raises(ValueError, match="could not find nn file {} please run precompute_knns".format(path).replace(".", r"\.")):
        D.ContrastiveSegDataset(str(tmp_path), "directory", None, "train", D.image_transform(R), D.label_transform(R), _cfg(tmp_path, R),
                                num_neighbors=K, mask=True, pos_images=True, pos_labels=True)
    nns, written = _nns(tmp_path, n, R)
    assert written == path
    ds = D.ContrastiveSegDataset(str(tmp_path), "directory", None, "train", D.image_transform(R), D.label_transform(R), _cfg(tmp_path, R, 9),
                                 num_neighbors=K, mask=True, pos_images=True, pos_labels=True)
    assert len(ds) == n and ds.n_classes == 9 and ds.feature_cache_file == path
    np.random.seed(0)
    torch.manual_seed(0)
    for ind in range(n):
        it = ds[ind]
        assert set(it) == {"ind", "img", "label", "img_pos", "ind_pos", "mask", "label_pos", "mask_pos"}
        assert it["ind"] == ind and int(it["ind_pos"]) in set(nns[ind, 1:K + 1].tolist())
        for k in ("img", "img_pos"):
            assert it[k].dtype == torch.float32 and tuple(it[k].shape) == (3, R, R)
        for k in ("label", "label_pos"):
            assert it[k].dtype == torch.int64 and tuple(it[k].shape) == (R, R)
        for k in ("mask", "mask_pos"):
            assert it[k].dtype == torch.float32 and tuple(it[k].shape) == (1, R, R)
        assert torch.equal(it["mask"][0], (it["label"] > 0).float()) and torch.equal(it["mask_pos"][0], (it["label_pos"] > 0).float())
    batch = next(iter(torch.utils.data.DataLoader(ds, 2, shuffle=False)))
    assert tuple(batch["img"].shape) == (2, 3, R, R) and tuple(batch["mask"].shape) == (2, 1, R, R) and batch["ind_pos"].dtype == torch.int64
    # without positives the table is not needed (the val loader); a crop_type with "directory" stays refused
    val = D.ContrastiveSegDataset(str(tmp_path), "directory", None, "train", D.image_transform(6), D.label_transform(6), _cfg(tmp_path, 6),
                                  mask=True)
    assert set(val[0]) == {"ind", "img", "label", "mask"}
    with pytest.raises(ValueError):
        D.ContrastiveSegDataset(str(tmp_path), "directory", "five", "train", D.image_transform(6), D.label_transform(6), _cfg(tmp_path, 6))


@pytest.mark.parametrize("crop", ["center", "random"])
def test_contrastive_directory_dataset_follows_the_reference_draw_order(tmp_path, crop):
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    imgs, labs = files(tmp_path, NAME, "train")
    n, res, K = len(HOST_SIZES), 6, 3
    nns, _ = _nns(tmp_path, n, res)
    ds = D.ContrastiveSegDataset(str(tmp_path), "directory", None, "train", D.image_transform(res, crop), D.label_transform(res, crop),
                                 _cfg(tmp_path, res), num_neighbors=K, mask=True, pos_images=True, pos_labels=True)

    def load(i, seed):
        rgb, lab = open_pair(imgs, labs, i)
        random.seed(seed)
        torch.manual_seed(seed)
        img = D.image_transform(res, crop)(rgb)
        random.seed(seed)
        torch.manual_seed(seed)
        return img, D.label_transform(res, crop)(lab)[0]

    for ind in range(n):
        np.random.seed(100 + ind)
        torch.manual_seed(200 + ind)
        got = ds[ind]
        state_after = torch.get_rng_state()
        # 1. dataset[ind] with its numpy seed, 2. torch.randint for the neighbour, 3. dataset[ind_pos], 4. the item's seed
        np.random.seed(100 + ind)
        torch.manual_seed(200 + ind)
        img, lab = load(ind, int(np.random.randint(2147483647)))
        r = torch.randint(low=1, high=K + 1, size=[]).item()
        ind_pos = nns[ind][r]
        img_p, lab_p = load(ind_pos, int(np.random.randint(2147483647)))
        seed = np.random.randint(2147483647)
        assert got["ind_pos"] == ind_pos
        for a, b in ((got["img"], img), (got["label"], lab), (got["img_pos"], img_p), (got["label_pos"], lab_p)):
            assert torch.equal(a, b)
        assert torch.equal(got["mask"][0], (lab > 0).float()) and torch.equal(got["mask_pos"][0], (lab_p > 0).float())
        assert torch.equal(state_after, torch.manual_seed(int(seed)).get_state())


@pytest.mark.parametrize("R", [6, 224])
def test_a_store_res_reduction_leaves_the_transform_bitwise_unchanged(tmp_path, R):
    """DeviceImageStore.from_directory(store_res=R) keeps data._resize(im, R): the transform at R of the reduced image is the
    transform of the original, for the centre crop and for any explicit origin."""
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    imgs, labs = files(tmp_path, NAME, "train")
    rng = np.random.default_rng(R)
    for i in range(len(imgs)):
        rgb, lab = open_pair(imgs, labs, i)
        small, small_lab = D._resize(rgb, R), D._resize(lab, R)
        assert min(small.size) == R and small.size == small_lab.size == D.resized_size(rgb.size[0], rgb.size[1], R)
        assert D.resized_size(small.size[0], small.size[1], R) == small.size            # left alone the second time
        assert torch.equal(bits(D.image_transform(R)(small)), bits(D.image_transform(R)(rgb)))
        assert torch.equal(D.label_transform(R)(small_lab), D.label_transform(R)(lab))
        nw, nh = small.size
        for _ in range(3):
            origin = (int(rng.integers(0, nh - R + 1)), int(rng.integers(0, nw - R + 1)))
            a, b = restated_item(small, small_lab, R, origin), restated_item(rgb, lab, R, origin)
            assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_directory_store_sizing_from_the_headers(tmp_path):
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    px = sum(h * w for h, w in HOST_SIZES)
    assert DD.directory_bytes(str(tmp_path), NAME, "train") == 4 * px
    # images above store_res shrink to it; the 1 x 9 one is kept (its upscale is left to prepare's index maps)
    reduced = sum(nw * nh for nw, nh in ((w, h) if min(w, h) <= 6 else D.resized_size(w, h, 6) for h, w in HOST_SIZES))
    assert reduced == 6 * 7 + 7 * 6 + 1 * 9 + 6 * 8
    assert DD.directory_bytes(str(tmp_path), NAME, "train", store_res=6) == 4 * reduced and reduced < px
    with pytest.raises(DD.StoreTooLarge, match=r"\(4 images\) and the budget is"):
        DD.DeviceImageStore.from_directory(str(tmp_path), NAME, "train", device="cpu", max_bytes=4 * px - 1)
    with pytest.raises(DD.StoreTooLarge, match=r"\(4 images, reduced to store_res = 6\) and the budget is"):
        DD.DeviceImageStore.from_directory(str(tmp_path), NAME, "train", device="cpu", max_bytes=4 * reduced - 1, store_res=6)
    shutil.rmtree(join(str(tmp_path), NAME, "labels"))
    assert DD.directory_bytes(str(tmp_path), NAME, "train") == 3 * px                    # no label arena


def test_a_reduced_store_keeps_the_reduced_bytes_and_refuses_another_resolution(tmp_path):
    write_folder(tmp_path, NAME, "train", HOST_SIZES)
    imgs, labs = files(tmp_path, NAME, "train")
    store = DD.DeviceImageStore.from_directory(str(tmp_path), NAME, "train", device="cpu", store_res=6)
    assert store.kind == "directory" and store.store_res == 6 and len(store) == len(imgs)
    assert store.nbytes == DD.directory_bytes(str(tmp_path), NAME, "train", store_res=6) == store.images.numel() + store.labels.numel()
    for i in range(len(imgs)):
        rgb, lab = open_pair(imgs, labs, i)
        h, w, o = int(store.h[i]), int(store.w[i]), int(store.label_offsets[i])
        small = min(rgb.size) <= 6                                   # kept as it is: a store never upscales
        assert np.array_equal(store.images[3 * o:3 * (o + h * w)].numpy().reshape(h, w, 3), np.asarray(rgb if small else D._resize(rgb, 6)))
        assert np.array_equal(store.labels[o:o + h * w].numpy().reshape(h, w), np.asarray(lab if small else D._resize(lab, 6)))
    with pytest.raises(ValueError, match="store_res = 6 and serves that resolution only, not R = 8"):
        store.table(8)
    rec = store.table(6)["records"]
    big = np.minimum(rec["h"], rec["w"]) >= 6
    assert (np.minimum(rec["nh"], rec["nw"]) == 6).all() and (rec["nh"] == rec["h"])[big].all() and (rec["nw"] == rec["w"])[big].all()
    assert big.sum() == 3 and tuple(rec[~big][["h", "w"]][0]) == (1, 9)
    shutil.rmtree(join(str(tmp_path), NAME, "labels"))
    bare = DD.DeviceImageStore.from_directory(str(tmp_path), NAME, "train", device="cpu")
    assert bare.labels is None and bare.nbytes == bare.images.numel() and bare.table(6)["desc"][3] == sum(h * w for h, w in HOST_SIZES)


def test_new_symbols_are_exported_and_the_abi_version_stays(tmp_path):
    from stego_amd import capi
    lib = capi.load()
    assert lib.stego_abi_version() == 7
    for name in ("stego_data_prepare_dir", "stego_salience_coords"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    assert b"salience" in lib.stego_error_string(capi.SALIENCE_ERR_SIZE) and b"salience" in lib.stego_error_string(capi.SALIENCE_ERR_SAMPLES)


def _aligned_buffer():
    buf = (ctypes.c_uint8 * 4096)()
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_prepare_dir_rejects_a_bad_descriptor_before_any_launch():
    """Host checks of stego_data_prepare_dir: they return before the device is touched (no GPU on this machine)."""
    from stego_amd import capi
    lib = capi.load()
    buf, p16 = _aligned_buffer()

    def call(desc, **kw):
        args = dict(items=p16, img_arena=p16, label_arena=p16, map_pool=p16, lut=p16, index=p16, origin=None, img=p16, label=p16, mask=p16)
        args.update(kw)
        return lib.stego_data_prepare_dir(ctypes.byref(desc), *args.values(), None)

    good = dict(N=4, R=8, n_items=3, img_arena_bytes=900, label_arena_bytes=300, map_pool_len=22)
    for k, v, code in [("R", 0, capi.DATA_ERR_RES), ("R", capi.DATA_MAX_RES + 1, capi.DATA_ERR_RES), ("N", 0, capi.DATA_ERR_COUNT),
                       ("N", capi.DATA_MAX_N + 1, capi.DATA_ERR_COUNT), ("n_items", 0, capi.DATA_ERR_COUNT),
                       ("n_items", 2 ** 31, capi.DATA_ERR_COUNT), ("img_arena_bytes", -1, capi.DATA_ERR_RANGE),
                       ("map_pool_len", -1, capi.DATA_ERR_RANGE)]:
        assert call(capi.data_desc(**dict(good, **{k: v}))) == code, (k, v)
        assert call(capi.data_desc(**dict(good, **{k: v})), label_arena=None) == code, (k, v)
    for name in ("items", "img_arena", "map_pool", "lut", "index", "img", "label", "mask"):
        assert call(capi.data_desc(**good), **{name: None}) == 1, name                 # STEGO_ERR_NULL (label_arena alone may be NULL)
    for name in ("img", "label", "mask", "index"):                                     # STEGO_ERR_ALIGN: 16-byte stores at R % 4 == 0
        assert call(capi.data_desc(**good), **{name: p16 + 4}) == 5, name
    odd = dict(good, R=7)                                                              # one pixel per lane: element alignment
    assert call(capi.data_desc(**odd), mask=p16 + 2) == 5 and call(capi.data_desc(**odd), img=p16 + 2) == 5
    assert call(capi.data_desc(**odd), label=p16 + 4) == 5 and call(capi.data_desc(**odd), origin=p16 + 2) == 5
    assert lib.stego_data_prepare_dir(None, *([p16] * 6), None, p16, p16, p16, None) == 1


def test_salience_coords_rejects_bad_arguments_before_any_launch():
    from stego_amd import capi
    lib = capi.load()
    buf, p16 = _aligned_buffer()

    def call(desc, **kw):
        args = dict(mask1=p16, mask2=p16, u=p16, u_mix=p16, reg1=p16, reg2=p16, coords1=p16, coords2=p16)
        args.update(kw)
        return lib.stego_salience_coords(ctypes.byref(desc), *args.values(), None)

    def desc(B=2, H=8, W=8, S=3, dtype=capi.SALIENCE_F32):
        return capi.StegoSalienceDesc(B, H, W, S, dtype)

    assert call(desc(S=0)) == capi.SALIENCE_ERR_SAMPLES and call(desc(S=17)) == capi.SALIENCE_ERR_SAMPLES
    assert call(desc(H=1024, W=1025)) == capi.SALIENCE_ERR_SIZE and call(desc(H=2 ** 20 + 1, W=1)) == capi.SALIENCE_ERR_SIZE
    assert call(desc(H=65536, W=65536)) == capi.SALIENCE_ERR_SIZE                     # the product does not wrap
    assert call(desc(B=0)) == capi.SALIENCE_ERR_SIZE and call(desc(B=65536)) == capi.SALIENCE_ERR_SIZE
    assert call(desc(H=0)) == capi.SALIENCE_ERR_SIZE and call(desc(W=0)) == capi.SALIENCE_ERR_SIZE
    assert call(desc(dtype=2)) == capi.SALIENCE_ERR_DTYPE
    for name in ("mask1", "mask2", "u", "u_mix", "reg1", "reg2", "coords1", "coords2"):
        assert call(desc(), **{name: None}) == 1, name                                 # STEGO_ERR_NULL
        assert call(desc(), **{name: p16 + 2}) == 5, name                              # STEGO_ERR_ALIGN
    assert lib.stego_salience_coords(None, *([p16] * 8), None) == 1
    assert not capi.salience_covers(4, 1024, 1025, 11) and not capi.salience_covers(4, 8, 8, 17) and capi.salience_covers(4, 224, 224, 11)

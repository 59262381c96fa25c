"""stego_amd.eval_segmentation's preprocessing against the reference's get_transform(res, _, "center") (src/utils.py:164-183):
torchvision Resize(res, NEAREST) - short side to res, long side truncated, no resize when the short side is res already - then
CenterCrop(res), on hand-computed pixels of small non-square images and their labels."""
import numpy as np
import torch
from PIL import Image

from stego_amd import eval_segmentation as E


def _rgb(w, h):
    """Pixel (x, y) = (x, y, 10 x + y): every pixel tells where it came from."""
    a = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            a[y, x] = (x, y, 10 * x + y)
    return Image.fromarray(a, "RGB")


def _label(w, h):
    return Image.fromarray((np.arange(w)[None, :] * 10 + np.arange(h)[:, None]).astype(np.uint8), "L")


def _src_xy(img_t):
    """Undo Normalize and ToTensor: the source (x, y) of every output pixel."""
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    v = torch.round((img_t * std + mean) * 255).to(torch.int64)
    return v[0].numpy(), v[1].numpy()


def test_wide_image_resized_with_truncated_long_side_then_centre_cropped():
    # 8 x 5 to res 3: the long side is int(3 * 8 / 5) = int(4.8) = 4 (rounding would give 5); NEAREST picks source columns
    # floor((i + 0.5) * 8 / 4) = 1, 3, 5, 7 and rows floor((j + 0.5) * 5 / 3) = 0, 2, 4; the centre crop's left offset is
    # int(round(0.5)) = 0 -> columns 1, 3, 5
    x, y = _src_xy(E.image_transform(3)(_rgb(8, 5)))
    np.testing.assert_array_equal(x, np.array([[1, 3, 5]] * 3))
    np.testing.assert_array_equal(y, np.array([[0, 0, 0], [2, 2, 2], [4, 4, 4]]))
    lab = E.label_transform(3)(_label(8, 5))
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (1, 3, 3)
    np.testing.assert_array_equal(lab[0].numpy(), 10 * x + y)


def test_tall_image_and_short_side_already_at_res():
    # 4 x 9 to res 4: the short side is 4 already - no resize; the crop's top offset is int(round(2.5)) = 2 (round half to even)
    x, y = _src_xy(E.image_transform(4)(_rgb(4, 9)))
    np.testing.assert_array_equal(x, np.tile(np.arange(4), (4, 1)))
    np.testing.assert_array_equal(y, np.tile(np.arange(2, 6)[:, None], (1, 4)))
    np.testing.assert_array_equal(E.label_transform(4)(_label(4, 9))[0].numpy(), 10 * x + y)
    # 5 x 11 to res 3: long side int(3 * 11 / 5) = 6; rows floor((j + 0.5) * 11 / 6) = 0, 2, 4, 6, 8, 10, crop top int(round(1.5)) = 2
    x, y = _src_xy(E.image_transform(3)(_rgb(5, 11)))
    np.testing.assert_array_equal(x, np.tile([0, 2, 4], (3, 1)))
    np.testing.assert_array_equal(y, np.tile(np.array([4, 6, 8])[:, None], (1, 3)))


def test_image_values_are_totensor_then_normalize():
    im = Image.fromarray(np.array([[[0, 128, 255]]], np.uint8), "RGB")
    t = E.image_transform(1)(im)
    expect = (torch.tensor([0, 128, 255], dtype=torch.float32) / 255 - torch.tensor([0.485, 0.456, 0.406])) / torch.tensor([0.229, 0.224, 0.225])
    torch.testing.assert_close(t[:, 0, 0], expect, rtol=0, atol=1e-6)


def test_make_loader_reads_the_cropped_val_split_through_the_transforms(tmp_path):
    """my_app's loader: the val split of a cropped tree (non-square crops) comes out resized and centre-cropped like the reference's."""
    import types
    from os.path import join
    from stego_amd.data import crop_dir, write_cropped
    g = torch.Generator().manual_seed(0)
    items = [(torch.rand(3, 20, 34, generator=g), torch.randint(-1, 5, (20, 34), generator=g)) for _ in range(2)]
    assert write_cropped(str(tmp_path), "cocostuff27", "five", 0.5, "val", items) == 10
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(dataset_name="cocostuff27", crop_type="five", crop_ratio=0.5), n_classes=27)
    cfg = types.SimpleNamespace(pytorch_data_dir=str(tmp_path), res=6, batch_size=2, num_workers=0)
    loader = E.make_loader(cfg, model)
    img, label, mask = next(iter(loader))
    assert tuple(img.shape) == (4, 3, 6, 6) and tuple(label.shape) == (4, 6, 6)
    d = crop_dir(str(tmp_path), "cocostuff27", "five", 0.5)
    with Image.open(join(d, "img", "val", "0.jpg")) as im:           # a 17 x 10 crop
        assert im.size == (17, 10)
        torch.testing.assert_close(img[0], E.image_transform(6)(im.convert("RGB")), rtol=0, atol=0)
    with Image.open(join(d, "label", "val", "0.png")) as lb:
        np.testing.assert_array_equal(label[0].numpy(), E.label_transform(6)(lb)[0].numpy() - 1)

"""python -m stego_amd.find_objects index=.../regions/index.npz image=NAME x=... y=... k=8 [out=matches.json]

Where else in a folder is an object like the one under this pixel?  The demo (save_regions=True save_region_index=True) wrote the region
tables, the id maps and `regions/index.npz`; this looks up the region under (x, y) in the image's id map (regions.read_id_map, named by
`regions/NAME.json`), searches the index for the k most similar regions by cosine (RegionIndex.search) and prints the matches as one
JSON document: the query, and per match image, region id, label, area, box and similarity.  It writes no pictures."""
import json
import os
import sys
from os.path import dirname, join

import torch

from .region_descriptors import RegionIndex, region_at
from .regions import read_id_map
from .train_segmentation import load_config

FIND_CONFIG = join(dirname(__file__), "configs", "find_config.yml")


def my_app(cfg):
    """-> the dict that is printed: {"query": {...}, "matches": [{"image", "region", "label", "area", "box", "similarity"}]}."""
    if not cfg.image:
        raise ValueError("image=NAME is required: the file name of the query image")
    index = RegionIndex.load(cfg.index)
    regions_dir = dirname(os.path.abspath(cfg.index))
    stem = os.path.splitext(cfg.image)[0]
    with open(join(regions_dir, stem + ".json")) as f:
        id_map = json.load(f)["id_map"]
    ids = read_id_map(join(dirname(regions_dir), "region_ids", id_map))
    region = region_at(ids, 0, int(cfg.x), int(cfg.y))
    if region < 0:
        raise ValueError("no region under pixel (%d, %d) of %s (a %d x %d map)" % (int(cfg.x), int(cfg.y), cfg.image, ids.shape[1], ids.shape[0]))
    row = index.row_of(cfg.image, region)
    device = getattr(cfg, "device", None) or ("cuda" if torch.cuda.is_available() else "cpu")
    rows, sims = index.search([row], k=int(cfg.k), min_area=int(getattr(cfg, "min_area", 0)),
                              other_images_only=bool(getattr(cfg, "other_images_only", True)), device=device)
    result = {"query": dict(index.row_info(row), x=int(cfg.x), y=int(cfg.y), pooled=index.pooled),
              "matches": [dict(index.row_info(r), similarity=float(s)) for r, s in zip(rows[0], sims[0]) if r >= 0]}
    print(json.dumps(result))
    if getattr(cfg, "out", None):
        with open(cfg.out, "w") as f:
            json.dump(result, f)
    return result


if __name__ == "__main__":
    my_app(load_config(FIND_CONFIG, overrides=sys.argv[1:]))

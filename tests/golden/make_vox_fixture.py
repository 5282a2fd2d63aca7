"""Derived test input for the GPU: the tree BoxTree::load_vox_file (restated in voxelhex_amd/csrc/vox.cpp) builds from
the reference's own model asset whisp/assets/models/gingerbread_house_by_kirra_luan.vox (brick_dim 8, a 2048^3 tree),
flattened and stored as compressed arrays, so that the GPU tests trace the reference's real model against the oracle
without importing it first. The asset itself is stored next to it (xz-compressed, tests/_models.py); its SHA-256 is
recorded, and tests/test_vox.py rebuilds the tree from the asset and checks it equals this fixture.

usage: python tests/golden/make_vox_fixture.py  ->  tests/golden/gingerbread_bd8.npz
"""
import hashlib
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SRC = "gingerbread_house_by_kirra_luan.vox"  # a tests/_models.py name
OUT = os.path.join(ROOT, "tests", "golden", "gingerbread_bd8.npz")
FIELDS = ("node_type", "node_ocbits", "node_children", "voxels", "solid_values", "color_palette", "data_palette")


def build(path, brick_dim=8):
    import voxelhex_amd as vhx
    flat = vhx.BoxTree.load_vox_file(path, brick_dim).flatten()
    arrays = {k: np.array(getattr(flat, k), copy=True) for k in FIELDS}
    arrays["sizes"] = np.array([flat.desc.boxtree_size, flat.desc.brick_dim], np.uint32)
    return arrays


def save_npz_lzma(path, arrays):
    """np.savez_compressed with LZMA members (numpy.load reads them): deflate leaves this tree above 1 MiB."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, a in arrays.items():
            with z.open(k + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def main():
    from tests._models import model_bytes, unpack_model
    with tempfile.TemporaryDirectory() as d:
        arrays = build(unpack_model(SRC, d))
    sha = hashlib.sha256(model_bytes(SRC)).hexdigest()
    save_npz_lzma(OUT, dict(arrays, source_sha256=np.array(sha)))
    print(OUT, os.path.getsize(OUT), "bytes; source", sha)


if __name__ == "__main__":
    main()

"""Small class-folder datasets for the classifier's device patch dataset (sr355.patches.LabeledPatches) and the defects loader to read:
seeded random-noise PNGs, so that any wrongly addressed pixel differs, and the class-map pickle."""
import os
import pickle

import numpy as np
from PIL import Image

# frame (h, w), patch, stride: the edges of sr_gather_warp_patches (see test_labeled_patches_gpu.py for what each one hits)
GEOMETRIES = (((37, 53), 11, 5), ((32, 32), 32, 16), ((150, 130), 96, 48), ((40, 36), 8, 4))
CLASS_DIRS = ("defect", "ok")           # class ids 1 and 0


def write_tree(root, n_images, hw, seed=0):
    """n_images random RGB PNGs of size hw, alternating between the two class folders of <root>/hr, and <root>/class_labels_map.pkl
    ({basename: class id}).  The files' basenames sort across the folders, so the loader's order (by basename) interleaves them.
    -> (hr_root, class_map_path, frames uint8 [N,H,W,3] in the loader's order, labels int64 [N])."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n_images, hw[0], hw[1], 3), dtype=np.uint8)
    hr_root = os.path.join(str(root), "hr")
    labels, class_map = np.zeros(n_images, np.int64), {}
    for i in range(n_images):
        folder = CLASS_DIRS[i % 2]
        os.makedirs(os.path.join(hr_root, folder), exist_ok=True)
        name = f"img_{i:02d}.png"
        Image.fromarray(frames[i]).save(os.path.join(hr_root, folder, name))
        labels[i] = 1 - i % 2
        class_map[name] = int(labels[i])
    class_map_path = os.path.join(str(root), "class_labels_map.pkl")
    with open(class_map_path, "wb") as f:
        pickle.dump(class_map, f)
    return hr_root, class_map_path, frames, labels


def walk(hw, patch, stride):
    """The defects loader's (i, j) walk over one frame: the unpadded extents."""
    return [(i, j) for i in range(0, hw[0] - patch + 1, stride) for j in range(0, hw[1] - patch + 1, stride)]

"""The classifier's device patch dataset, host side (sr355.patches.LabeledPatches), without a GPU: the window table, the labels and the shapes
against load_defects_dataset_as_patches on class-folder PNG trees (tests/labeled_patches_ref.py), the subset / view algebra that makes
train_test_split work on the view, the byte counts, and every error -- all before anything touches a device."""
import os
import pickle

import numpy as np
import pytest
from PIL import Image

import labeled_patches_ref as R
from sr355.patches import LabeledPatches, LabeledView, labeled_dataset, window_table_defects
from SRModels.loading_methods import load_defects_dataset_as_patches


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Nothing in this file may reach for a device context."""
    import sr355

    def boom(*a, **k):
        raise AssertionError("a device context was requested")

    monkeypatch.setattr(sr355.Context, "get", staticmethod(boom))


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_table_labels_and_shape_equal_the_loader(geom, tmp_path):
    hw, patch, stride = geom
    hr_root, cmap, frames, labels = R.write_tree(tmp_path, 3, hw, seed=sum(hw))
    X, y = load_defects_dataset_as_patches(hr_root, patch, stride, cmap)
    ds = LabeledPatches.from_dirs(hr_root, patch, stride, cmap)
    walk = R.walk(hw, patch, stride)
    assert len(walk) >= 1 and len(ds) == len(X) == len(y) == 3 * len(walk)
    assert ds.y.dtype == np.int64 and np.array_equal(ds.y, y)
    assert np.array_equal(ds.windows, np.array([(n, i, j) for n in range(3) for i, j in walk], np.int32))
    assert ds.windows.dtype == np.int32 and np.array_equal(ds.windows, window_table_defects(3, hw, patch, stride))
    assert ds.X.shape == X.shape and ds.X.dtype == X.dtype and ds.X.ndim == X.ndim == 4 and len(ds.X) == len(X)
    assert ds.frame_size == hw and ds.patch_size == patch
    # the stack is the decoded files in the loader's order, and no window reaches past the unpadded frame
    assert np.array_equal(ds._s.frames, frames)
    assert (ds.windows[:, 1] + patch).max() <= hw[0] and (ds.windows[:, 2] + patch).max() <= hw[1]
    # the loader's values at the table's windows, from the uint8 stack (what the gather computes per element)
    k = len(ds) // 2
    n, i, j = ds.windows[k]
    assert np.array_equal(frames[n, i:i + patch, j:j + patch].astype(np.float32) / 255.0, X[k])
    # the loader's switch returns the same dataset's view and labels
    Xv, yv = load_defects_dataset_as_patches(hr_root, patch, stride, cmap, on_device=True)
    assert isinstance(Xv, LabeledView) and labeled_dataset(Xv) is Xv.ds and labeled_dataset(X) is None
    assert np.array_equal(Xv.ds.windows, ds.windows) and np.array_equal(yv, y) and yv.dtype == np.int64 and Xv.shape == X.shape


def test_geometry_edges_are_what_the_cases_claim():
    (a, pa, sa), (b, pb, sb), (c, pc, sc), (d, pd, sd) = R.GEOMETRIES
    wa = window_table_defects(1, a, pa, sa)
    assert (pa * pa * 3) % 4 != 0 and (wa[:, 1] + pa).max() < a[0] and (wa[:, 2] + pa).max() < a[1]       # the last rows / columns belong to no window
    assert len(window_table_defects(1, b, pb, sb)) == 1 and b == (pb, pb)                                   # the origin clamp range is one point
    assert (pc, sc) == (96, 48) and len(window_table_defects(3, c, pc, sc)) == 6
    wd = window_table_defects(1, d, pd, sd)
    assert len(wd) == 72 and np.any((wd[:, 1] > 0) & (wd[:, 2] > 0) & (wd[:, 1] + pd < d[0]) & (wd[:, 2] + pd < d[1]))   # interior windows


def test_reference_geometry_gives_64_windows_per_frame():
    assert len(window_table_defects(2, (478, 478), 96, 48)) == 2 * 64


def _dataset(n=4, hw=(20, 26), patch=8, stride=4, seed=3):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)
    return LabeledPatches.from_stacks(frames, np.arange(n) % 2, patch, stride), frames


def test_subsets_and_view_indexing_compose():
    ds, _ = _dataset()
    n = len(ds)
    assert n == 4 * 4 * 5
    rng = np.random.default_rng(0)
    a = rng.permutation(n)[:50]
    b = rng.permutation(50)[:17]
    assert np.array_equal(ds.X[a][b].ds.windows, ds.X[a[b]].ds.windows) and np.array_equal(ds.X[a][b].ds.windows, ds.windows[a[b]])
    assert np.array_equal(ds.subset(a).subset(b).y, ds.y[a[b]])
    assert ds.X[a].ds._s is ds._s and ds.X[a].shape == (50, 8, 8, 3) and len(ds.X[a]) == 50
    for sl in (slice(5, 31), slice(None, None, 3), slice(60, None), slice(10, 2, -2), slice(0, 0)):
        v = ds.X[sl]
        assert isinstance(v, LabeledView) and np.array_equal(v.ds.windows, ds.windows[sl]) and np.array_equal(v.ds.y, ds.y[sl])
    assert np.array_equal(ds.X[a][3:9].ds.windows, ds.windows[a[3:9]])
    assert np.array_equal(ds.X[a.astype(np.int32)].ds.windows, ds.windows[a])
    for bad in (np.array([0, n]), np.array([-1]), np.array([0.5]), np.zeros((2, 2), int)):
        with pytest.raises(ValueError):
            ds.X[bad]
    with pytest.raises(ValueError):
        ds.subset(a).subset(np.array([50]))


def test_byte_counts_are_the_stack_plus_the_tables():
    ds, frames = _dataset()
    table, labels = ds.windows, ds.y
    assert ds.host_bytes() == frames.nbytes + table.nbytes + labels.nbytes
    assert ds.device_bytes() == frames.nbytes + table.nbytes == 4 * 20 * 26 * 3 + 80 * 3 * 4
    sub = ds.subset(np.arange(10))
    assert sub.host_bytes() == ds.host_bytes() + 10 * 8 and sub.device_bytes() == ds.device_bytes()
    f32 = LabeledPatches.from_stacks(frames.astype(np.float32) / 255.0, np.zeros(4, int), 8, 4)
    assert f32.device_bytes() == 4 * frames.nbytes + table.nbytes
    # the issue's arithmetic: 313 frames of 478 x 478, 96 / 48 -> 20 032 patches of 110 592 B against 214.5 MB of distinct pixels
    n_patches = 313 * 64
    assert n_patches == 20032 and 96 * 96 * 3 * 4 == 110592 and round(313 * 478 * 478 * 3 / 1e6, 1) == 214.5


def test_errors_are_raised_on_the_host(tmp_path):
    hr_root, cmap, frames, labels = R.write_tree(tmp_path, 3, (20, 24), seed=1)
    # the loader's validation, with its messages, from both entry points
    for call in (lambda **k: LabeledPatches.from_dirs(**k), lambda **k: load_defects_dataset_as_patches(on_device=True, **k)):
        with pytest.raises(ValueError, match="HR root directory must exist."):
            call(hr_root=str(tmp_path / "nowhere"), patch_size=8, stride=4, class_map_path=cmap)
        with pytest.raises(ValueError, match="HR root path must be a directory."):
            call(hr_root=cmap, patch_size=8, stride=4, class_map_path=cmap)
        with pytest.raises(ValueError, match="patch_size must be positive int."):
            call(hr_root=hr_root, patch_size=0, stride=4, class_map_path=cmap)
        with pytest.raises(ValueError, match="stride must be positive int."):
            call(hr_root=hr_root, patch_size=8, stride=2.0, class_map_path=cmap)
        with pytest.raises(ValueError, match="class_map_path must be a non-empty string."):
            call(hr_root=hr_root, patch_size=8, stride=4, class_map_path=None)
        with pytest.raises(FileNotFoundError):
            call(hr_root=hr_root, patch_size=8, stride=4, class_map_path=str(tmp_path / "missing.pkl"))
        empty = tmp_path / "empty"
        empty.mkdir(exist_ok=True)
        with pytest.raises(ValueError, match="No images found under HR root directory."):
            call(hr_root=str(empty), patch_size=8, stride=4, class_map_path=cmap)
        # the patch exceeds the frame: no windows
        with pytest.raises(ValueError, match="exceeds"):
            call(hr_root=hr_root, patch_size=21, stride=4, class_map_path=cmap)
    # a basename the map lacks
    short = str(tmp_path / "short.pkl")
    with open(short, "wb") as f:
        pickle.dump({"img_00.png": 1, "img_01.png": 0}, f)
    with pytest.raises(KeyError, match="img_02.png"):
        LabeledPatches.from_dirs(hr_root, 8, 4, short)
    # the first file whose size differs from the first is named
    odd = os.path.join(hr_root, R.CLASS_DIRS[1], "img_01.png")
    Image.fromarray(np.zeros((20, 25, 3), np.uint8)).save(odd)
    with pytest.raises(ValueError, match="img_01.png"):
        LabeledPatches.from_dirs(hr_root, 8, 4, cmap)
    # stacks
    with pytest.raises(ValueError):
        LabeledPatches.from_stacks(frames.astype(np.float64), labels, 8, 4)
    with pytest.raises(ValueError):
        LabeledPatches.from_stacks(frames[0], labels, 8, 4)
    with pytest.raises(ValueError):
        LabeledPatches.from_stacks(frames, labels[:2], 8, 4)
    with pytest.raises(ValueError):
        LabeledPatches.from_stacks(frames, labels.astype(np.float32), 8, 4)
    with pytest.raises(ValueError, match="exceeds"):
        LabeledPatches.from_stacks(frames, labels, 25, 4)
    with pytest.raises(ValueError):
        LabeledPatches.from_device(frames, labels, channel_order="gbr", patch_size=8, stride=4)
    with pytest.raises(ValueError):
        window_table_defects(1, (20, 24), 8, True)


def test_train_test_split_works_on_the_view():
    ms = pytest.importorskip("sklearn.model_selection")
    ds, _ = _dataset(n=5)
    X, y = ds.X, ds.y
    Xtr, Xte, ytr, yte = ms.train_test_split(X, y, test_size=0.2, random_state=42)
    itr, ite = ms.train_test_split(np.arange(len(X)), test_size=0.2, random_state=42)
    assert isinstance(Xtr, LabeledView) and isinstance(Xte, LabeledView) and len(Xtr) == len(itr) and len(Xte) == len(ite)
    assert np.array_equal(Xtr.ds.windows, ds.windows[itr]) and np.array_equal(Xte.ds.windows, ds.windows[ite])
    assert np.array_equal(ytr, y[itr]) and np.array_equal(yte, y[ite]) and np.array_equal(Xtr.ds.y, ytr) and np.array_equal(Xte.ds.y, yte)

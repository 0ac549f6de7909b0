"""FineTunedVGG16._augment_params: the device fit draws its augmentation parameters on the host, and they must be the same draws, in the same
order, as the host path's _augment made before the device path existed (VGG16_model.py:129-134)."""
import numpy as np
import pytest


def _old_draws(rng, n, h, w, rotation_range=20, width_shift_range=0.2, height_shift_range=0.2, horizontal_flip=True):
    """The draw sequence of the pre-device _augment, restated: per image uniform angle, uniform ty, uniform tx, then random() for the flip."""
    rots, offs, flips = [], [], []
    for _ in range(n):
        th = np.deg2rad(rng.uniform(-rotation_range, rotation_range))
        ty, tx = rng.uniform(-height_shift_range, height_shift_range) * h, rng.uniform(-width_shift_range, width_shift_range) * w
        c, s_ = np.cos(th), np.sin(th)
        rot = np.array([[c, -s_], [s_, c]])
        centre = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
        offs.append(centre - rot @ centre + np.array([ty, tx]))
        rots.append(rot)
        flips.append(bool(horizontal_flip and rng.random() < 0.5))
    return np.array(rots), np.array(offs), np.array(flips)


@pytest.mark.parametrize("n,h,w,flip", [(1, 32, 32, True), (7, 128, 128, True), (5, 37, 53, True), (4, 16, 16, False), (0, 8, 8, True)])
def test_augment_params_consume_the_generator_as_augment_did(n, h, w, flip):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    a, b = np.random.default_rng(123), np.random.default_rng(123)
    rot, off, fl = FineTunedVGG16._augment_params(a, n, h, w, horizontal_flip=flip)
    rot0, off0, fl0 = _old_draws(b, n, h, w, horizontal_flip=flip)
    assert a.bit_generator.state == b.bit_generator.state
    assert rot.shape == (n, 2, 2) and off.shape == (n, 2) and fl.shape == (n,)
    if n:
        assert np.array_equal(rot, rot0) and np.array_equal(off, off0) and np.array_equal(fl, fl0)
    assert a.random() == b.random()


def test_augment_keeps_its_output():
    """_augment on the factored-out parameters: the same scipy transform per image and channel, then the flip."""
    from scipy import ndimage
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    x = np.random.default_rng(0).uniform(0, 1, (3, 12, 10, 3)).astype(np.float32)
    got = FineTunedVGG16._augment(x, np.random.default_rng(4))
    rng = np.random.default_rng(4)
    rot, off, fl = _old_draws(rng, 3, 12, 10)
    for i in range(3):
        ref = np.stack([ndimage.affine_transform(x[i, :, :, c], rot[i], offset=off[i], order=1, mode="nearest") for c in range(3)], -1)
        if fl[i]:
            ref = ref[:, ::-1]
        assert np.array_equal(got[i], ref)


def test_warp_params_split_fp64_into_hi_and_lo():
    from sr355.runtime import Context
    rng = np.random.default_rng(2)
    rot, off = rng.normal(size=(4, 2, 2)) * 3, rng.normal(size=(4, 2)) * 50
    p = Context.warp_params(rot, off, [True, False, True, False])
    assert p.shape == (4, 16) and p.dtype == np.float32
    v = np.concatenate([rot.reshape(4, 4), off], 1)
    assert np.abs(p[:, :6].astype(np.float64) + p[:, 6:12] - v).max() <= 1e-12 * np.abs(v).max()
    assert list(p[:, 12]) == [1, 0, 1, 0] and not p[:, 13:].any()
    with pytest.raises(ValueError):
        Context.warp_params(rot, off, [True])

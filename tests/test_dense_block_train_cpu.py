"""Training a G = 8 dense block on the LDS-resident kernels, the parts that need no GPU: the packer's layout restated in NumPy round-trips,
the option checkers refuse what they must, and an fp32 evaluation of the arithmetic contract keeps the share cap the GPU test sets."""
import numpy as np
import pytest
import torch

import dense_block_train_ref as R


def test_forward_fragments_follow_the_host_packers_rule():
    """block_pack_weights (csrc/dense_block.hip): fragment (tap, c, n) of conv i at db_frag0 + (tap * nc + c) * nb + n; lane l, element j = cin 32 c + 8 (l >> 4) + j,
    cout 16 n + (l & 15); zero beyond the conv's own cins / couts.  Restated here element by element, without the vectorised indexing of the reference."""
    ws = R.block_weights(3)
    frags, bias = R.pack_forward_np(ws)
    assert frags.shape == (207, 64, 8) and bias.shape == (128,)
    rng = np.random.default_rng(0)
    for i in range(5):
        cin, cout, nc, nb = R.CIN[i], R.COUT[i], (2 if i == 0 else 3), (1 if i < 4 else 4)
        frag0 = 0 if i == 0 else 9 * (2 + 3 * (i - 1))
        kb = R.bf16_bits_np(ws[i][0])
        for _ in range(400):
            tap, c, n, l, j = rng.integers(9), rng.integers(nc), rng.integers(nb), rng.integers(64), rng.integers(8)
            ci, co = 32 * c + 8 * (l >> 4) + j, 16 * n + (l & 15)
            want = kb[tap // 3, tap % 3, ci, co] if ci < cin and co < cout else 0
            assert frags[frag0 + (tap * nc + c) * nb + n, l, j] == want
        off = 16 * i if i < 4 else 64
        assert np.array_equal(bias[off:off + cout], ws[i][1]) and not bias[off + cout:off + (16 if i < 4 else 64)].any()
    # every real weight appears exactly once: the count of non-zero entries is that of the kernels
    assert int((frags != 0).sum()) == sum(int((R.bf16_bits_np(k) != 0).sum()) for k, _ in ws)


def test_backward_fragments_unpack_to_the_rotated_transposed_kernels():
    ws = R.block_weights(4)
    frags = R.pack_backward_np(ws)
    assert frags.shape == (288, 64, 8)
    outs, pad_zero = R.unpack_backward_np(frags)
    assert pad_zero
    for i in range(5):
        kb = R.bf16_bits_np(ws[i][0])                                       # [3,3,cin,cout]
        want = kb[::-1, ::-1].transpose(0, 1, 3, 2)                          # rotated by 180 degrees, cin and cout swapped
        assert np.array_equal(outs[i], want), i
    assert int((frags != 0).sum()) == sum(int((R.bf16_bits_np(k) != 0).sum()) for k, _ in ws)
    # the K rows a growth conv does not have (lanes 16 .. 63) are zero in every one of its fragments
    assert not frags[108:, 16:, :].any()


def test_option_checkers():
    from sr355.gan_train import DENSE_BLOCK_IMPLS, Tape, check_dense_block_impl, trunk_layers_lds
    import inspect
    from sr355.gan_train import ESRGANTrainer
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    assert DENSE_BLOCK_IMPLS[0] == "layers"
    assert inspect.signature(ESRGANTrainer.__init__).parameters["dense_block_impl"].default == "layers"
    assert inspect.signature(Tape.__init__).parameters["dense_block_impl"].default == "layers"
    assert inspect.signature(ESRGAN.__init__).parameters["train_dense_block"].default == "layers"
    assert check_dense_block_impl("layers", "f32") == "layers" and check_dense_block_impl("lds", "bf16") == "lds"
    with pytest.raises(ValueError, match="dense_block_impl must be one of"):
        check_dense_block_impl("fused")
    with pytest.raises(ValueError, match="needs train_dtype='bf16'"):
        check_dense_block_impl("lds", "f32")
    with pytest.raises(ValueError, match="needs train_dtype='bf16'"):
        ESRGAN(train_dense_block="lds")
    with pytest.raises(ValueError, match="dense_block_impl must be one of"):
        ESRGAN(train_dtype="bf16", train_dense_block="LDS")
    assert ESRGAN(train_dtype="bf16", train_dense_block="lds").train_dense_block == "lds"
    assert ESRGAN().train_dense_block == "layers"
    # a block that is not G = 8 is refused and named: the first offending layer
    w = R.weight_sets(nb=2)["he_normal"]
    assert len(trunk_layers_lds(w, 2)) == 30
    bad = dict(w)
    k, b = w["rrdb_1_dense2_conv3"]
    bad["rrdb_1_dense2_conv3"] = (np.zeros((3, 3, 80, 16), np.float32), np.zeros(16, np.float32))
    bad["rrdb_1_dense3_conv1"] = (np.zeros((3, 3, 64, 32), np.float32), np.zeros(32, np.float32))
    with pytest.raises(ValueError, match="rrdb_1_dense2_conv3 has 16 growth channels"):
        trunk_layers_lds(bad, 2)
    with pytest.raises(ValueError, match="rrdb_1_dense2_conv3"):
        ESRGANTrainer(None, bad, None, None, 2, 2, train_dtype="bf16", dense_block_impl="lds")      # before anything is uploaded: no context needed
    with pytest.raises(ValueError, match="needs train_dtype='bf16'"):
        ESRGANTrainer(None, w, None, None, 2, 2, dense_block_impl="lds")


@pytest.mark.parametrize("case", R.CASES + [(2, 24, 24, 0)], ids=lambda c: "x".join(map(str, c)))
def test_an_fp32_evaluation_keeps_the_share_cap(case):
    """The GPU test allows 1e-2 of the elements of a stage to differ from the once-rounded fp64 reference (fp32 accumulation may carry a value across a rounding
    boundary).  On the same inputs torch's fp32 convs -- another summation order than the kernel's -- stay below that cap at every stage, teacher-forced like the GPU
    test: the cap is one that fp32 arithmetic itself keeps."""
    B, H, W, _ = case
    ws = R.block_weights(7)
    x, r_in, dY = R.case_inputs(B, H, W)
    worst = 0.0
    for a5, bx, r in ((0.2, 1.0, None), (0.04, 0.2, r_in)):
        F64, out64 = R.block_forward(ws, x, a5, bx, r)
        F32, out32 = R.block_forward(ws, x, a5, bx, r, dtype=torch.float32)
        # slice by slice from the fp32 run's own stored prefix
        for convs in (R.forward_checks(ws, F32, out32, a5, bx, r),):
            for label, got, v, _ in convs:
                share = R.differing_share(got, R.rb(v))
                worst = max(worst, share)
                print(f"{case} a5={a5} forward {label}: {share:.2e} of the elements differ")
                assert share <= 1e-2, label
        st32, dz32, dX32 = R.block_backward(ws, F64, dY, a5, bx, dtype=torch.float32)
        stages = torch.stack([st32[5], st32[4], st32[3], st32[2]])
        # (the contract's G keeps slice k itself beyond cin_k; the kernel's dump holds dz there: make the fp32 run look like a dump)
        for j, k in ((1, 4), (2, 3), (3, 2)):
            for kk in range(4, k - 1, -1):
                stages[j][..., R.CIN[kk - 1]:R.CIN[kk - 1] + 8] = dz32[..., (kk - 1) * 8:kk * 8]
        convs, exact = R.backward_checks(ws, F64, dY, stages, dz32, dX32, a5, bx)
        for label, got, v, _ in convs:
            share = R.differing_share(got, R.rb(v))
            worst = max(worst, share)
            print(f"{case} a5={a5} backward {label}: {share:.2e} of the elements differ")
            assert share <= 1e-2, label
        for label, got, ref in exact:
            assert torch.equal(got.double(), ref.double()), label
    print(f"{case}: the largest share over all stages is {worst:.2e}")

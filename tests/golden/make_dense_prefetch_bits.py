"""Writes tests/golden/dense_prefetch_bits.json: a SHA-256 per tap (conv1, conv2, conv3, conv5 of every dense block) of the fused
dense-block kernels' outputs at the shapes, masks and weights of tests/test_dense_prefetch_bits_gpu.py, which restates nothing: the cases
and the hashing are imported from it.  Needs a GPU and a built library; run from the repository root ON THE COMMIT WHOSE BITS ARE THE
REFERENCE (the file in the tree was recorded on the commit before the kernels' operand reads were carried across granule barriers):
    python tests/golden/make_dense_prefetch_bits.py [output path]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_dense_prefetch_bits_gpu as T
    from sr355 import Context
    ctx = Context.get(0)
    out = {"seed": T.SEED, "num_blocks": T.NUM_BLOCKS, "sha256": {}}
    for case, mask_name in T.PARAMS:
        out["sha256"][T.key_of(case, mask_name)] = T.tap_hashes(ctx, case, mask_name)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dense_prefetch_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out["sha256"]), "cases")


if __name__ == "__main__":
    main()

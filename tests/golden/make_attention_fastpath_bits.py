"""Writes tests/golden/attention_fastpath_bits.json: per case of tests/attention_fastpath_cases.py the SHA-256 of the bf16 bytes the
SelfAttention core stored (attention_ref.run_core), and the raw bits (base64 of little-endian int16 [B,N,32]) where N <= 256.  The cases
and the hashing are imported, nothing is restated.  Needs a GPU and a built library; run from the repository root ON THE COMMIT WHOSE BITS
ARE THE REFERENCE (the file in the tree was recorded on the commit before attn_bf16_kernel's unguarded groups got their own loop):
    python tests/golden/make_attention_fastpath_bits.py [output path]"""
import base64
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import attention_fastpath_cases as F
    import attention_ref as R
    from sr355 import Context
    ctx = Context.get(0)
    out = {"sha256": {}, "bits": {}, "shapes": {}}
    for name in F.names_smallest_first():
        c = F.cases()[name]
        runs = [F.stored_bits(R.run_core(ctx, c["k"], c["q"], c["v"], "bf16")) for _ in range(2)]
        assert (runs[0] == runs[1]).all(), f"{name}: two runs of the same inputs differ"
        out["sha256"][name] = F.sha256_of(runs[0])
        out["shapes"][name] = [int(c["k"].shape[0]), int(c["n"])]
        if c["n"] <= F.RAW_BITS_MAX_N:
            out["bits"][name] = base64.b64encode(runs[0].tobytes()).decode("ascii")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "attention_fastpath_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out["sha256"]), "cases")


if __name__ == "__main__":
    main()

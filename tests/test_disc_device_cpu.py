"""The device-side discriminator update's C ABI (csrc/disc_train.hip) without a GPU: the two entry points are declared in include/sr355.h,
bound in sr355/_lib.py and exported by the built library; sr_sn_desc has the C compiler's layout; without a context they refuse."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_spectral_norm_bucket", "sr_disc_head_step")


def test_new_symbols_are_declared_bound_and_exported():
    from sr355 import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr355.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", txt))
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["sr_spectral_norm_bucket"][1]) == 8 and len(_lib.SIGNATURES["sr_disc_head_step"][1]) == 16
    # no context: invalid, and nothing is dereferenced
    assert lib.sr_spectral_norm_bucket(None, None, 0, None, 0, None, 0, None) == _lib.SR_ERR_INVALID
    assert lib.sr_disc_head_step(None, None, 1, 1, 1, 256, 256, 1, None, 1.0, None, None, None, None, 0, None) == _lib.SR_ERR_INVALID


def test_sn_desc_layout_is_the_headers(tmp_path):
    from sr355 import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sr355.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(sr_sn_desc), offsetof(sr_sn_desc, koff), offsetof(sr_sn_desc, K), offsetof(sr_sn_desc, Cout),\n'
                   '         offsetof(sr_sn_desc, uoff));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.SnDesc
    assert got == [ctypes.sizeof(D), D.koff.offset, D.K.offset, D.Cout.offset, D.uoff.offset]


def test_descriptor_table_of_a_bucket():
    """Context.spectral_norm_table needs no device: offsets follow ParamBucket's order (kernel then bias, layer after layer), K is the product
    of all axes but the last, the u vectors follow each other in the order of the names given."""
    from sr355.runtime import Context

    class Bucket:
        shapes = {"a": [(3, 3, 3, 64), (64,)], "b": [(3, 3, 5, 7), (7,)], "c": [(256, 1), (1,)]}
    table, u_len = Context.spectral_norm_table(Bucket, ["a", "c", "b"])
    rows = [(d.koff, d.K, d.Cout, d.uoff) for d in table]
    assert rows == [(0, 27, 64, 0), (27 * 64 + 64 + 45 * 7 + 7, 256, 1, 64), (27 * 64 + 64, 45, 7, 65)] and u_len == 72

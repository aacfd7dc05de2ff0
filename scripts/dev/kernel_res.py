"""Print, per tile / SMA kernel inside a libbt build, its register, scratch and LDS counts (the
metadata tests/test_kernel_resources.py checks), its instruction count and a hash of its
instruction listing (llvm-objdump, without addresses, comments, `<symbol+off>` annotations and
the zero padding `...` after a section's last kernel). Two builds whose rows agree run the same
machine code in these kernels: run it on libbt.so and on a reference build (scripts/
build_ref_lib.sh) and diff the output. A second argument, a regular expression searched in the
kernel's symbol name, lists other kernels instead (the lane kernels: 'replay_kernel|wf_|pf_|gram_').
usage: python scripts/dev/kernel_res.py [path/to/libbt.so [name-regex]]"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import test_kernel_resources as T  # noqa: E402


def listings():
    """kernel symbol -> its stripped instruction lines, over every code object of T.LIB."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in T._code_objects(d):
            dis = subprocess.run([os.path.join(T.LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950",
                                  "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = T._FUNC.match(line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif cur is not None and line[:1].isspace():  # an instruction line
                    line = re.sub(r"<[^>]*>", "", line.split("//")[0]).strip()
                    if line and line != "...":
                        cur.append(line)
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1:
        T.LIB = sys.argv[1]
    keep = re.compile(sys.argv[2] if len(sys.argv) > 2 else "tile_kernel|sma|seg_combine")
    lst = listings()
    for name, d in sorted(T._kernels().items()):
        if not keep.search(name):
            continue
        ins = lst.get(name, [])
        print(f"{name[:70]:70s} vgpr {d.get('vgpr_count')} sgpr {d.get('sgpr_count')} "
              f"spill {d.get('vgpr_spill_count')} priv {d.get('private_segment_fixed_size')} "
              f"lds {d.get('group_segment_fixed_size')} insts {len(ins)} "
              f"sha {hashlib.sha256(chr(10).join(ins).encode()).hexdigest()[:16]}")

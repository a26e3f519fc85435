#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libmlearn.so.

  tools/compare_device_code.py A/libmlearn.so B/libmlearn.so

For a host-only change the two libraries must hold the same kernels: the
same kernel symbol names, per kernel the same code bytes, and per kernel the
same .vgpr_count / .sgpr_count / .group_segment_fixed_size /
.private_segment_fixed_size.  Each library is copied to a temporary folder
and unbundled there (llvm-objdump --offloading); symbols, section headers
and notes are read with llvm-readelf.  Hashes and counts only.  Exit status
0 when the device code is the same, 1 when it differs.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True,
                          capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(lib, os.path.join(d, "lib.so"))
    run("llvm-objdump", "--offloading", "lib.so", cwd=d)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith("gfx950"))


def kernels(obj):
    """{kernel name: (sha256 of its code bytes, size, metadata tuple)}"""
    data = open(obj, "rb").read()
    text = None
    for line in run("llvm-readelf", "-S", "-W", obj).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = tuple(int(x, 16) for x in m.groups())  # address, file offset, size
    funcs, kds = {}, set()
    for line in run("llvm-readelf", "-s", "-W", obj).splitlines():
        p = line.split()
        if len(p) != 8 or not p[0].endswith(":"):
            continue
        if p[3] == "OBJECT" and p[7].endswith(".kd"):
            kds.add(p[7][:-3])
        elif p[3] == "FUNC":
            funcs[p[7]] = (int(p[1], 16), int(p[2]))
    meta = {}
    for entry in re.split(r"(?m)^  - ", run("llvm-readelf", "--notes", "-W", obj)):
        name = re.search(r"(?m)^    \.name:\s+(\S+)", entry)
        if name:
            meta[name.group(1)] = tuple(
                int(re.search(r"(?m)^    %s:\s+(\d+)" % re.escape(f), entry).group(1)) for f in FIELDS)
    out = {}
    for k in kds:
        addr, size = funcs[k]
        assert text[0] <= addr and addr + size <= text[0] + text[2], k
        off = text[1] + addr - text[0]
        out[k] = (hashlib.sha256(data[off:off + size]).hexdigest(), size, meta[k])
    return out, hashlib.sha256(data).hexdigest()


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for lib in sys.argv[1:]:
            objs = [kernels(o) for o in code_objects(lib, tmp)]
            allk = {}
            for ks, _ in objs:
                assert not set(ks) & set(allk), "a kernel name in two code objects"
                allk.update(ks)
            sides.append((objs, allk))
            print("%s: %d code objects, kernel descriptors %s = %d" %
                  (lib, len(objs), " + ".join(str(len(ks)) for ks, _ in objs), len(allk)))
    (oa, ka), (ob, kb) = sides
    same_obj = sum(1 for (_, ha), (_, hb) in zip(oa, ob) if ha == hb) if len(oa) == len(ob) else 0
    print("code objects with equal SHA-256: %d of %d" % (same_obj, len(oa)))
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    code = sorted(k for k in set(ka) & set(kb) if ka[k][:2] != kb[k][:2])
    meta = sorted(k for k in set(ka) & set(kb) if ka[k][2] != kb[k][2])
    print("kernels only in the first: %d, only in the second: %d" % (len(only_a), len(only_b)))
    print("kernels in both: %d, code bytes differ: %d, %s differ: %d" %
          (len(set(ka) & set(kb)), len(code), " / ".join(FIELDS), len(meta)))
    for title, names in (("only in the first", only_a), ("only in the second", only_b),
                         ("code differs", code), ("metadata differs", meta)):
        for k in names:
            print("  %s: %s" % (title, k))
    bad = bool(only_a or only_b or code or meta)
    print("device code: %s" % ("DIFFERS" if bad else "the same"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

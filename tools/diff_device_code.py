"""Device code of two builds, kernel by kernel: python tools/diff_device_code.py OLD_DIR NEW_DIR  (directories of *.hip.o objects, as
build() leaves them in csrc/build).  For every translation unit the gfx950 code object is taken out of both objects
(llvm-objdump --offloading), disassembled, and compared function by function: instructions (addresses and encodings apart) and the
resource metadata (registers, LDS, scratch).  One line per translation unit, plus every kernel that differs."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".sgpr_count", ".vgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count",
        ".vgpr_spill_count", ".max_flat_workgroup_size", ".kernarg_segment_size", ".wavefront_size")


def code_object(obj, tmp):
    d = os.path.join(tmp, os.path.basename(obj) + ("%d" % len(os.listdir(tmp))))
    os.makedirs(d)
    copy = shutil.copy(obj, d)  # (the bundles are written next to the object)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, stdout=subprocess.DEVNULL)
    found = [f for f in glob.glob(os.path.join(d, "*")) if "gfx950" in f]
    return found[0] if found else None


def functions(co):
    """{symbol: [instruction text]} of a code object."""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                         capture_output=True, text=True).stdout
    fns, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line.strip())
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line.strip()))
    return fns


def metadata(co):
    """{kernel: {field: value}} from the code object's notes."""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        s = line.strip()
        if s.startswith("- .agpr_count") or s.startswith("- .args"):  # (the first key of a kernel's record)
            cur = {}
        m = re.match(r"^-?\s*(\.[a-z_]+):\s*(\S+)$", s)
        if m and cur is not None:
            if m.group(1) in META:
                cur[m.group(1)] = m.group(2)
            if m.group(1) == ".symbol":
                kernels[m.group(2).strip("'\"")[:-3]] = cur
    return kernels


def main(old_dir, new_dir):
    worst = 0
    with tempfile.TemporaryDirectory() as tmp:
        for old in sorted(glob.glob(os.path.join(old_dir, "*.hip.o"))):
            new = os.path.join(new_dir, os.path.basename(old))
            co_a, co_b = code_object(old, tmp), code_object(new, tmp)
            if co_a is None and co_b is None:
                print("%-28s no device code" % os.path.basename(old))
                continue
            fa, fb, ma, mb = functions(co_a), functions(co_b), metadata(co_a), metadata(co_b)
            diff = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k) or ma.get(k) != mb.get(k))
            print("%-28s %3d functions (%d kernels with metadata), %d differ" % (os.path.basename(old), len(fb), len(mb), len(diff)))
            for k in diff:
                what = "only in old" if k not in fb else "only in new" if k not in fa else "instructions" if fa[k] != fb[k] else "metadata"
                print("    %s: %s (%d -> %d instructions; %s -> %s)" % (k, what, len(fa.get(k, [])), len(fb.get(k, [])), ma.get(k), mb.get(k)))
            worst = max(worst, len(diff))
    return 1 if worst else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

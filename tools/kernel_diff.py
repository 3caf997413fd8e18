"""Do two builds of the device code agree?  Compiles every compu_amd/csrc/*.hip of two source trees to gfx950 assembly (no GPU; the
flags of tools/spill_audit.py) and prints SAME or DIFF per function; exit status 1 on any DIFF or any function on one side only.

  python tools/kernel_diff.py A B   # A, B: the root of a source tree, or a git revision of this repository (HEAD, a hash)
  python tools/kernel_diff.py A B -- -DCHIP_STATS ...   # what follows `--` is appended to every compile of both trees

Compared per function: the lines between `; -- Begin function NAME` and `; -- End function` without comments, without the
.section / .file / .loc / .ident / .p2align lines, local labels reduced to their number within the function; and per kernel its
amdhsa.kernels entry: register counts, both spill counts, LDS and scratch sizes.  It reports agreement only, never which
instructions occur."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_tree(arg, tmp, extra):
    """(file, assembly text) of every .hip of a source tree or git revision, compiled with the flags `extra` as well; brotli.hip's
    generated include (build.sh) is made here"""
    if not os.path.isdir(arg):
        tar = subprocess.run(["git", "-C", ROOT, "archive", arg, "compu_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        arg = tmp
    src = os.path.join(arg, "compu_amd", "csrc")
    os.makedirs(os.path.join(tmp, "asm", "build"))
    with open(os.path.join(src, "brotli_dict.bin"), "rb") as f, open(os.path.join(tmp, "asm", "build", "brotli_dict.inc"), "w") as inc:
        inc.write(",".join(str(x) for x in f.read()) + ",\n")

    def one(f):
        out = os.path.join(tmp, "asm", f[:-4] + ".s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", os.path.join(tmp, "asm"), "-o", out,
                        os.path.join(src, f)] + extra, check=True, stderr=subprocess.DEVNULL)
        return f, open(out).read()

    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(one, sorted(f for f in os.listdir(src) if f.endswith(".hip"))))


def functions(units):
    """name -> (normalised body, metadata of a kernel or None); a name that several files define gets the file's beside it"""
    found = []
    for f, asm in units:
        meta = {}
        for entry in asm.partition("amdhsa.kernels:")[2].split("\n  - ")[1:]:
            fields = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", entry, re.M))
            if "name" in fields:  # (the split also yields the amdhsa.version list behind the kernels)
                meta[fields["name"]] = tuple(fields.get(k) for k in META)
        for m in re.finditer(r"; -- Begin function (\S+)\n(.*?); -- End function", asm, re.S):
            body = []
            for line in m.group(2).splitlines():
                line = re.sub(r"\.L(BB|func_end|func_begin)\d+_?", r".L\1", line.split(";")[0]).strip()
                if line and not line.startswith((".section", ".file", ".loc", ".ident", ".p2align")):
                    body.append(line)
            found.append((m.group(1), f, (body, meta.get(m.group(1)))))
    names = [n for n, _, _ in found]
    return {(n, f if names.count(n) > 1 else ""): v for n, f, v in found}


def main():
    extra = sys.argv[4:] if sys.argv[3:4] == ["--"] else []
    if len(sys.argv) != 3 and sys.argv[3:4] != ["--"]:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = functions(compile_tree(sys.argv[1], ta, extra)), functions(compile_tree(sys.argv[2], tb, extra))
    keys = sorted(set(a) | set(b))
    plain = subprocess.run(["c++filt"], input="\n".join(n for n, _ in keys), capture_output=True, text=True).stdout.splitlines()
    bad = 0
    for (key, short) in sorted(zip(keys, plain), key=lambda kp: (kp[1], kp[0][1])):
        word = "SAME" if a.get(key) == b.get(key) else "DIFF" if key in a and key in b else "ONLY IN " + sys.argv[1 if key in a else 2]
        bad += word != "SAME"
        kind = "kernel" if (a.get(key) or b.get(key))[1] else "function"
        print(word, kind, short.replace("(anonymous namespace)::", "").split("(")[0], key[1])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

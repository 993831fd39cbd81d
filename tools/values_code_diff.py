"""Compare the gfx950 machine code of every kernel a base revision already had with the working tree's.

Each translation unit the base's build.sh lists is compiled, in the base (a `git archive` of --base) and in the working tree,
with build.sh's flags.  The gfx950 code object of each object file is taken out of its .hip_fatbin bundle and disassembled
with llvm-objdump -d; every symbol's instructions are compared with the addresses and encodings stripped (and the filler behind a symbol's last instruction dropped: zero words, and the s_nop run that pads the unit's last symbol).  Kernels only the
working tree has (new units, new instantiations) are counted, not compared.

    python tools/values_code_diff.py [--base HEAD] [--units xhist_extrema,xhist_meanvar,...] [--jobs 8]

Prints one line per unit and exits 1 if any pre-existing symbol's code differs.  Runs without a GPU."""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def units_of(tree):
    text = open(os.path.join(tree, "xhistogram_amd", "csrc", "build.sh")).read()
    return re.search(r"^tus=\(([^)]*)\)", text, re.M).group(1).split()


def disassemble(tree, unit, work):
    """{symbol: [instruction text]} of one unit's gfx950 code object"""
    obj = os.path.join(work, unit + ".o")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc")] + FLAGS + ["-c", "-o", obj, os.path.join(tree, "xhistogram_amd", "csrc", unit + ".hip")],
                   check=True, capture_output=True)
    fat = os.path.join(work, unit + ".fatbin")
    co = os.path.join(work, unit + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET,
                    "--output=" + co], check=True, capture_output=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    syms, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip() or line.startswith("Disassembly"):
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()  # (the address and the encoding are in the trailing comment)
        if ins:
            enc = re.search(r"//\s*[0-9A-Fa-f]+:\s*([0-9A-Fa-f ]+)$", line)
            cur.append((re.sub(r"\s+", " ", ins), ins == "..." or (bool(enc) and not enc.group(1).replace(" ", "").strip("0"))))  # ("...": objdump's run of zero words)
    # Words of zeros behind a symbol's last instruction are the filler up to the next symbol's alignment (they disassemble as
    # v_cndmask_b32 v0, s0, v0, vcc): how many there are depends on what follows the symbol, not on its code.  The same holds
    # for the run of s_nop 0 behind the s_endpgm of the unit's last symbol (the padding of the code section's end): a symbol
    # that another one now follows loses it.
    for name, body in syms.items():
        while True:
            n = len(body)
            while body and body[-1][1]:
                body.pop()
            k = len(body)
            while k and body[k - 1][0] == "s_nop 0":
                k -= 1
            if k and body[k - 1][0] == "s_endpgm":
                del body[k:]
            if len(body) == n:
                break
        syms[name] = [ins for ins, _ in body]
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD", help="git revision whose kernels must keep their code (default HEAD)")
    ap.add_argument("--units", default="", help="comma-separated units (default: every unit of the base's build.sh)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        arc = subprocess.run(["git", "-C", ROOT, "archive", a.base], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base], input=arc, check=True)
        units = a.units.split(",") if a.units else units_of(base)
        jobs = {}
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            for side, tree in (("base", base), ("tree", ROOT)):
                work = os.path.join(tmp, side + "_obj")
                os.makedirs(work)
                for u in units:
                    jobs[side, u] = ex.submit(disassemble, tree, u, work)
            res = {k: f.result() for k, f in jobs.items()}
    bad = 0
    for u in units:
        b, t = res["base", u], res["tree", u]
        missing = sorted(set(b) - set(t))
        differ = sorted(s for s in b if s in t and b[s] != t[s])
        new = len(set(t) - set(b))
        print("%-26s %4d symbols of the base: %d identical, %d differ, %d missing; %d new" % (
            u, len(b), len(b) - len(differ) - len(missing), len(differ), len(missing), new))
        for s in differ + missing:
            print("    " + s)
        bad += len(differ) + len(missing)
    print("RESULT: %s" % ("no difference in any pre-existing symbol" if not bad else "%d pre-existing symbols changed" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

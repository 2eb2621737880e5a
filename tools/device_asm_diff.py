"""Are two builds' device code the same, kernel for kernel?  python tools/device_asm_diff.py DIR_A DIR_B

DIR_A / DIR_B each hold bcnf_<unit>.s for every translation unit (bcnf_*.hip) of bcnf_amd/csrc, made on the two commits
with
  hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S -Iinclude bcnf_amd/csrc/bcnf_<unit>.hip -o DIR/bcnf_<unit>.s
Each file is split at its function symbols (instantiation order may move between builds), then per unit: the sets of
.amdhsa_kernel names are compared, and each function's text and each kernel's .amdhsa_* descriptor (registers, LDS,
scratch). Two things move with a function's position in the file and are normalised: the numbers of local labels
(.LBB<function>_<block>: renumbered by first appearance inside the function) and the `;` comments that name them.
Prints one line per unit; exit status 1 if anything differs.
"""
import glob
import os
import re
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "bcnf_amd", "csrc")
UNITS = tuple(sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(CSRC, "bcnf_*.hip"))))


def split(path):
    txt = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))
    bodies = {m.group(1): m.group(2)
              for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)}
    desc = {m.group(1): m.group(2)
            for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", txt, re.M | re.S)}
    return kernels, bodies, desc


def norm(body):
    body = re.sub(r"[ \t]*;[^\n]*", "", body)
    seen = {}
    body = re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), body)
    return re.sub(r"\n\s*\n", "\n", body)


def main(dir_a, dir_b):
    same = True
    for u in UNITS:
        ka, fa, da = split(os.path.join(dir_a, f"bcnf_{u}.s"))
        kb, fb, db = split(os.path.join(dir_b, f"bcnf_{u}.s"))
        line = f"bcnf_{u}.hip: {len(ka)} kernels / {len(kb)} kernels: "
        if ka != kb or set(fa) != set(fb):
            same = False
            line += f"sets differ: only A {sorted((ka - kb) | (set(fa) - set(fb)))}, only B {sorted((kb - ka) | (set(fb) - set(fa)))}"
        else:
            diff = sorted(k for k in fa if norm(fa[k]) != norm(fb[k]) or da.get(k) != db.get(k))
            same = same and not diff
            line += "identical" if not diff else "DIFFERENT: " + ", ".join(diff)
        print(line)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

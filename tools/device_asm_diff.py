"""Are two builds' device code the same, kernel for kernel?  python tools/device_asm_diff.py DIR_A DIR_B

DIR_A / DIR_B each hold bcnf_<unit>.s for every translation unit (bcnf_*.hip) of bcnf_amd/csrc on that commit, made
with
  hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S -Iinclude bcnf_amd/csrc/bcnf_<unit>.hip -o DIR/bcnf_<unit>.s
Each file is split at its function symbols (instantiation order may move between builds). A unit on one side may be
several on the other (bcnf_stack.hip became bcnf_stack*.hip), so the functions of all units are pooled per side and
compared by symbol -- kernels in anonymous namespaces keep their mangled names across files: the sets of
.amdhsa_kernel names, each function's text and each kernel's .amdhsa_* descriptor (registers, LDS, scratch). RENAMED
lists the symbols whose name changed on purpose (A's name -> B's). Two things move with a function's position in the
file and are normalised: the numbers of local labels (.LBB<function>_<block>: renumbered by first appearance inside
the function) and the `;` comments that name them.
Prints one line per unit of either side, then the symbols present on one side only; exit status 1 if anything differs
or a symbol is defined by two units of one side.
"""
import glob
import os
import re
import sys

# k_inverse<NH, true> -> k_inverse<NH>: the DROP parameter went with the eval arm nothing could launch
RENAMED = {f"_ZN12_GLOBAL__N_19k_inverseILi{nh}ELb1EEEv10BcnfLayoutPKfS3_S3_xPKlxPfPKm":
           f"_ZN12_GLOBAL__N_19k_inverseILi{nh}EEEv10BcnfLayoutPKfS3_S3_xPKlxPfPKm" for nh in range(1, 9)}


def split(path):
    txt = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))
    bodies = {m.group(1): m.group(2)
              for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)}
    desc = {m.group(1): m.group(2)
            for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", txt, re.M | re.S)}
    return kernels, bodies, desc


def norm(body, names=()):
    for a, b in names:
        body = body.replace(a, b)
    body = re.sub(r"[ \t]*;[^\n]*", "", body)
    seen = {}
    body = re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), body)
    return re.sub(r"\n\s*\n", "\n", body)


def pool(d, rename):
    """unit -> its symbols, and symbol -> (unit, is kernel, text, descriptor) over every bcnf_*.s of directory d."""
    units, syms, twice = {}, {}, []
    for path in sorted(glob.glob(os.path.join(d, "bcnf_*.s"))):
        u = os.path.basename(path)[:-2]
        kernels, bodies, desc = split(path)
        units[u] = (len(kernels), [rename.get(s, s) for s in bodies])
        for s, body in bodies.items():
            names = [(s, rename[s])] if s in rename else ()
            t = rename.get(s, s)
            if t in syms:
                twice.append(t)
            syms[t] = (u, s in kernels, norm(body, names), desc.get(s))
    return units, syms, twice


def main(dir_a, dir_b):
    ua, sa, twice_a = pool(dir_a, RENAMED)
    ub, sb, twice_b = pool(dir_b, {})
    differ = sorted(s for s in set(sa) & set(sb) if sa[s][1:] != sb[s][1:])
    for side, units, other in (("A", ua, sb), ("B", ub, sa)):
        for u, (nk, names) in units.items():
            homes = sorted({other[s][0] for s in names if s in other})
            bad = [s for s in names if s in differ]
            print(f"{side} {u}.hip: {nk} kernels, {len(names)} functions, on the other side in {', '.join(homes) or '-'}: "
                  + ("identical" if not bad else "DIFFERENT: " + ", ".join(bad)))
    only_a, only_b = sorted(set(sa) - set(sb)), sorted(set(sb) - set(sa))
    print(f"kernels: {sum(v[1] for v in sa.values())} / {sum(v[1] for v in sb.values())}; renamed {len(RENAMED)}")
    for side, only in (("A", only_a), ("B", only_b)):
        print(f"only {side} ({len(only)}):" + "".join("\n  " + s for s in only))
    for side, twice in (("A", twice_a), ("B", twice_b)):
        if twice:
            print(f"defined by two units of {side}: " + ", ".join(twice))
    return 1 if differ or only_a or only_b or twice_a or twice_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

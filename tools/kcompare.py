"""Compare the bond-scan kernels of two builds of the engine library (code-object
metadata and code bytes; no GPU needed): code size, VGPR / SGPR counts, spills,
scratch, LDS and kernel-argument size of every k_bonds* / k_rust_big_* kernel
that both hold, and whether its machine code is byte-identical.
    python tools/kcompare.py parent/libyuma_hip.so [this/libyuma_hip.so] [-v] [--all] [--by-code]
--all compares every kernel of the two code objects, not only the bond scans.
--by-code pairs the bond scans whose names do not pair (a template parameter
list that changed shape) by their code: the multisets of (code size, code
sha1, metadata) of the unpaired kernels of either side must be equal, and any
kernel left without a partner is printed. With --all, every other kernel is
still compared under its unchanged name.
k_bonds_elem's trailing history element type (HT = float, the default) is
dropped from a name before the two sides are matched, so that a library built
before that parameter existed pairs with one built after.
A k_bonds_elem<VARIANT, SH, FORM> name is printed with its form word as bit
names behind it, [VEC|RQ|...] (elem_form, form_names)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size", "kernarg_segment_size")
TAIL = "EEvNS_8BondArgsE"
EF = ("VEC", "RQ", "U16", "HS", "BF16", "SC", "MV", "RL", "RW", "RS")  # k_bonds_elem's form word, bit 0 first (yk::EF_*)
ELEM = re.compile(r"k_bonds_elemILi(\d)ENS_9ElemShapeI(.*?)EEELj(\d+)E(?=EEvNS_8ElemArgsI)")


def elem_form(name):
    """(variant, shape arguments, form word) of a k_bonds_elem<VARIANT, SH, FORM> name, else None"""
    m = ELEM.search(name)
    return (m.group(1), m.group(2), int(m.group(3))) if m else None


def form_names(form):
    return "|".join(n for i, n in enumerate(EF) if form >> i & 1) or "0"


def elem_forms(names, bit):
    """the k_bonds_elem names whose form word has the bit (a name of EF): name -> (variant, shape, form)"""
    return {k: f for k, f in ((k, elem_form(k)) for k in names) if f and f[2] >> EF.index(bit) & 1}


def with_form(name, clear, add=None):
    """the name with bit `clear` of its form word cleared and bit `add` set: a form's twin"""
    m = ELEM.search(name)
    form = int(m.group(3)) & ~(1 << EF.index(clear)) | (1 << EF.index(add) if add else 0)
    return f"{name[:m.start(3)]}{form}{name[m.end(3):]}"


def show(name):
    f = elem_form(name)
    return f"{name} [{form_names(f[2])}]" if f else name


def kernels(lib, every=False):
    """mangled name -> (code bytes, sha1 of the code, the metadata FIELDS) of
    the k_bonds* / k_rust_big_* kernels, or (every) of all kernels"""
    with tempfile.TemporaryDirectory() as t:
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={t}/fb", lib], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={t}/fb",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={t}/co"], check=True)
        run = lambda *a: subprocess.run(a, capture_output=True, text=True, check=True).stdout
        notes = run(f"{LLVM}/llvm-readobj", "--notes", f"{t}/co")
        m = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-SW", f"{t}/co"))
        addr, off = int(m.group(1), 16), int(m.group(2), 16)
        data = open(f"{t}/co", "rb").read()
        code = {}
        for line in run(f"{LLVM}/llvm-readelf", "-sW", f"{t}/co").splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC":
                o, n = off + int(f[1], 16) - addr, int(f[2])
                code[f[7]] = (n, hashlib.sha1(data[o:o + n]).hexdigest())
    out = {}
    for e in re.split(r"\n\s*- \.agpr_count", notes):
        m = re.search(r"\.name:\s+(\S+)", e)
        if not m or not (every or re.search(r"k_bonds|k_rust_big", m.group(1))):
            continue
        meta = tuple((re.search(r"\." + k + r":\s+(\d+)", e) or [None, "-"])[1] for k in FIELDS)
        out[m.group(1)] = code.get(m.group(1), (None, None)) + (meta,)
    return out


def key(name):
    # (One rewrite per template parameter k_bonds_elem once gained. From the form word on (<VARIANT, SH, FORM>) a
    # new option is a new bit and changes no existing name: no further rewrite is needed.)
    # <..., RW, RL> takes conditional_t<SH::RS, BondArgsRs, ElemArgs<SC, MV, RW, RL>>: the name of before the row
    # summary (an ElemShapeRs shape, BondArgsRs: only in a library that has it)
    name = re.sub(r"EEEvNSt11conditionalIXsrT0_2RSENS_10BondArgsRsENS\d+_(IXT8_ENS_10BondArgsRwE.*)E4typeE$",
                  r"EEEvNSt11conditional\1", name)
    # <..., SC, MV, RW = false, RL> takes ElemArgs<SC, MV, RW, RL>: the name of before the validator-row events (RW =
    # true, BondArgsRw: only in a library that has them)
    name = re.sub(r"Lb0E(Lb[01])EEEvNSt11conditionalIXT8_ENS_10BondArgsRwENS3_IXT9_ENS_10BondArgsRlE(.*)E4typeE$",
                  r"\1EEEvNSt11conditionalIXT8_ENS_10BondArgsRlE\2", name)
    # <..., SC, MV, RL = false> takes ElemArgs<SC, MV, RL>: the name of before the reset events (RL = true,
    # BondArgsRl: only in a library that has them)
    name = re.sub(r"Lb0EEEvNSt11conditionalIXT8_ENS_10BondArgsRlENS3_IXT7_ENS3_IXT6_ENS_12BondArgsScMvENS_10BondArgsMvEE"
                  r"4typeENS3_IXT6_ENS_10BondArgsScENS_8BondArgsEE4typeEE4typeEE4typeE$",
                  "EEvNSt11conditionalIXT7_ENS3_IXT6_ENS_12BondArgsScMvENS_10BondArgsMvEE4typeENS3_IXT6_"
                  "ENS_10BondArgsScENS_8BondArgsEE4typeEE4typeE", name)
    # <..., SC, MV = false> takes ElemArgs<SC, MV>: the name of before the bond movement (MV = true, BondArgsMv /
    # BondArgsScMv: only in a library that has it)
    name = re.sub(r"Lb0EEEvNSt11conditionalIXT7_ENS3_IXT6_ENS_12BondArgsScMvENS_10BondArgsMvEE4typeENS3_IXT6_"
                  r"ENS_10BondArgsScENS_8BondArgsEE4typeEE4typeE$",
                  "EEvNSt11conditionalIXT6_ENS_10BondArgsScENS_8BondArgsEE4typeE", name)
    # <..., HT, SC = false> takes conditional_t<SC, BondArgsSc, BondArgs>: the name of before the input
    # schedules (SC = true, BondArgsSc: only in a library that has them)
    name = re.sub(r"Lb0EEEvNSt11conditionalIXT\d+_ENS_10BondArgsScENS_8BondArgsEE4typeE$", TAIL, name)
    # <..., WT, HS, HT = float> ends in Lb0Ef / Lb1Ef; without HT the name ends in Lb0E / Lb1E
    if "k_bonds_elemI" in name and re.search(r"Lb[01]Ef" + TAIL + "$", name):
        return name[:-len("f" + TAIL)] + TAIL
    return name


def pair_by_code(A, B):
    """The bond scans of A and B that no name pairs, paired by (size, sha1,
    metadata): the pairs, and the kernels of either side left over."""
    scan = lambda k: re.search(r"k_bonds|k_rust_big", k)
    pool = {}
    for k in sorted(set(B) - set(A)):
        if scan(k):
            pool.setdefault(B[k], []).append(k)
    pairs, left = [], []
    for k in sorted(set(A) - set(B)):
        if not scan(k):
            continue
        if pool.get(A[k]):
            pairs.append((k, pool[A[k]].pop(0)))
        else:
            left.append(k)
    return pairs, left, sorted(k for ks in pool.values() for k in ks)


def main():
    every = "--all" in sys.argv
    args = [a for a in sys.argv[1:] if a not in ("-v", "--all", "--by-code")]
    a = kernels(args[0], every)
    b = kernels(args[1] if len(args) > 1 else os.path.join(ROOT, "yuma-simulation_amd", "lib", "libyuma_hip.so"), every)
    A = {key(k): v for k, v in a.items()}
    B = {key(k): v for k, v in b.items()}
    both = sorted(set(A) & set(B))
    meta = [k for k in both if (A[k][0], A[k][2]) != (B[k][0], B[k][2])]
    code = [k for k in both if A[k][1] != B[k][1]]
    print(f"{'all' if every else 'bond-scan'} kernels: {len(A)} in the first library, {len(B)} in the second, {len(both)} in both")
    print(f"  code size / registers / spills / scratch / LDS / kernarg differ: {len(meta)}")
    print(f"  machine code differs: {len(code)}")
    print(f"  only in the first: {len(set(A) - set(B))}")
    for k in sorted(set(meta) | set(code)):
        print("DIFF", show(k), A[k], B[k])
    head = "code " + " ".join(f.replace("_count", "").replace("_fixed_size", "").replace("_segment", "") for f in FIELDS)
    print(f"only in the second ({len(set(B) - set(A))}): {head}")
    for k in sorted(set(B) - set(A)):
        print(" ", show(k), B[k][0], *B[k][2])
    if "--by-code" in sys.argv:
        pairs, la, lb = pair_by_code(A, B)
        scans = lambda D: sum(1 for k in D if re.search(r"k_bonds|k_rust_big", k))
        print(f"bond-scan kernels: {scans(A)} in the first library, {scans(B)} in the second; "
              f"{scans(set(A) & set(B))} under the same name")
        print(f"bond scans paired by code (byte-identical, equal metadata): {len(pairs)}; "
              f"without a partner: {len(la)} of the first library, {len(lb)} of the second")
        for k in la:
            print("UNPAIRED first ", show(k), A[k][0], *A[k][2])
        for k in lb:
            print("UNPAIRED second", show(k), B[k][0], *B[k][2])
        if "-v" in sys.argv:
            for x, y in pairs:
                print("  PAIR", show(x), "\n      ", show(y))
    if "-v" in sys.argv:
        print(f"in both: {head}")
        for k in both:
            print(" ", show(k), A[k][0], *A[k][2])


if __name__ == "__main__":
    main()

"""The vector-memory waits of k_bonds_elem's event and summary forms, from the
library's gfx950 code object (no GPU needed): the RL (reset event) and RS (row
summary) forms beside their plain twins, and the RW (validator-row event) forms
beside their RL twins; a twin is the same name with the bit of the form word
cleared, or RW -> RL (kcompare.elem_forms, with_form).
For each pair it prints the s_waitcnt vmcnt(N) instructions inside the epoch
loop and outside it, the byte and dword loads, and the register report (VGPRs,
SGPRs, spills, scratch). The epoch loop is the largest backward-branch range
of the kernel (a conditional branch closes it; an unconditional one where
the exit test stands at the loop's head), with the out-of-line blocks that
branch back into it.
    python tools/kwaits.py [libyuma_hip.so] > profiles/row_resets/waitcnt.txt
A prefetch ring that is intact shows counted waits (vmcnt(N), N > 0) in the
loop; a vmcnt(0) in the loop that the twin lacks is a drain. A pair printed
with `loop [-]` has no loop the tool could find and must be read by hand."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kcompare  # noqa: E402

# The forms with a bit of k_bonds_elem's form word, each beside its twin: (title, bit, the twin's bit or None for
# the bit cleared, the twin's tag)
PAIRS = (("RL forms and their plain twins: s_waitcnt vmcnt(N) in the epoch loop and outside it;", "RL", None, "plain"),
         ("RW forms (validator-row events: both tables) and their RL twins", "RW", "RL", "RL   "),
         ("RS forms (the per-validator bond summary) and their plain twins", "RS", None, "plain"))


def disassemble(lib):
    """mangled name -> [(offset in the function, instruction text)]"""
    with tempfile.TemporaryDirectory() as t:
        subprocess.run([f"{kcompare.LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={t}/fb", lib], check=True)
        subprocess.run([f"{kcompare.LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={t}/fb",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={t}/co"], check=True)
        text = subprocess.run([f"{kcompare.LLVM}/llvm-objdump", "-d", f"{t}/co"], capture_output=True, text=True,
                              check=True).stdout
    out, cur, start = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            start, cur = int(m.group(1), 16), m.group(2)
            out[cur] = []
            continue
        m = re.match(r"^\s+\S.*?// ([0-9A-F]+):", line)
        if m and cur is not None:
            out[cur].append((int(m.group(1), 16) - start, line.strip()))
    return out


def target(text, name):
    m = re.search(r"<" + re.escape(name) + r"\+0x([0-9a-f]+)>", text) if "s_cbranch" in text or "s_branch" in text else None
    return int(m.group(1), 16) if m else None


def loop_ranges(ins, name):
    """The epoch loop as offset ranges: the largest backward-branch range (closed
    by s_cbranch_*, or by s_branch where the compiler rotated the exit test to the
    loop's head, as in the one-row flat Yuma 3 forms), and
    the out-of-line blocks behind it that the loop branches to and that branch
    back into it (the compiler parks rare blocks and, in the HS kernels, the
    refill blocks there)."""
    def largest(kind):
        r = (0, -1)
        for off, text in ins:
            t = target(text, name)
            if t is not None and kind in text and "_exec" not in text and t <= off and off - t > r[1] - r[0]:
                r = (t, off)
        return r

    # The largest range a conditional branch closes (not s_cbranch_exec*: those close loops over a wave's lanes,
    # never one over epochs); but where a larger range closed by an unconditional branch
    # lies apart from it, that one: the compiler rotated the epoch loop's exit test to its head, and the
    # conditional range is a loop of the prologue. (Where the unconditional range holds the conditional one, its
    # branch comes from an out-of-line block behind the loop, handled below.)
    best, alt = largest("s_cbranch"), largest("s_branch")
    if alt[1] - alt[0] > best[1] - best[0] and not (alt[0] <= best[0] and best[1] <= alt[1]):
        best = alt
    ranges = [best]
    inside = lambda o: any(lo <= o <= hi for lo, hi in ranges)
    offs = [o for o, _ in ins]
    changed = best[1] >= 0
    while changed:
        changed = False
        starts = sorted({t for o, x in ins if inside(o) for t in [target(x, name)] if t is not None and not inside(t)})
        for s in starts:
            if s not in offs:
                continue
            for o, x in ins[offs.index(s):]:
                if "s_endpgm" in x:
                    break
                t = target(x, name)
                if t is not None and "s_branch" in x and not inside(o):
                    if inside(t):
                        ranges.append((s, o))
                        changed = True
                    break
    return ranges


def waits(ins, name):
    ranges = loop_ranges(ins, name)
    inside, outside, loads, words = collections.Counter(), collections.Counter(), 0, 0
    for off, text in ins:
        m = re.search(r"s_waitcnt.*?vmcnt\((\d+)\)", text)
        if m:
            (inside if any(lo <= off <= hi for lo, hi in ranges) else outside)[f"vmcnt({m.group(1)})"] += 1
        loads += "global_load_ubyte" in text
        words += bool(re.search(r"global_load_dword\b", text))
    fmt = lambda c: " ".join(f"{k} x{v}" for k, v in sorted(c.items(), key=lambda kv: int(kv[0][6:-1]))) or "-"
    return f"loop [{fmt(inside)}]  outside [{fmt(outside)}]  byte loads {loads}  dword loads {words}"


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(kcompare.ROOT, "yuma-simulation_amd", "lib", "libyuma_hip.so")
    code, meta = disassemble(lib), kcompare.kernels(lib)
    for n, (title, bit, twin_bit, twin_tag) in enumerate(PAIRS):
        if n:
            print()
        print("k_bonds_elem " + title)
        if not n:
            print("registers: " + " ".join(kcompare.FIELDS))
        forms = kcompare.elem_forms(code, bit)
        for name in sorted(forms, key=lambda k: forms[k]):
            variant, shape, form = forms[name]
            print(f"variant {variant} shape {shape} form {kcompare.form_names(form)}")
            for tag, k in ((f"{bit}   ", name), (twin_tag, kcompare.with_form(name, bit, twin_bit))):
                if k in code:
                    print(f"  {tag} {waits(code[k], k)}  regs {' '.join(meta[k][2])}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""disasm_kernel.py — print the gfx950 disassembly of one kernel of
libnbxccl.so (exact mangled name, or a unique substring), plus an opcode
histogram with --hist. usage: disasm_kernel.py NAME [--hist] [--so PATH]

Compare mode: disasm_kernel.py --compare PARENT HEAD [--md OUT]
PARENT and HEAD are two builds of the library (or two gfx950 code objects of
one unit). Every kernel is compared instruction for instruction; a kernel
that differs is listed with both builds' instruction count, VGPRs, SGPR
spills, LDS and scratch bytes and its memory / LDS-DMA / LDS / atomic / wait /
barrier instruction counts, and is accepted only if scratch stays 0, LDS
bytes, memory, LDS-DMA and atomic counts are equal and the waves per SIMD its
VGPR count allows are unchanged. That step is min(8, 512 / VGPRs rounded up to
8): a SIMD has 8 wave slots, so a change below 65 VGPRs (41 -> 40, say) is no
step change here, though 512 / count alone would call it one. The counts are
of instructions in the code, not of instructions run. Kernels outside the kReduce* / kWide*
families are the control: any difference there fails. Exit status 0 when
every kernel is identical or accepted."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def code_objects(so):
    head = open(so, "rb").read(20)
    if head[:4] == b"\x7fELF" and int.from_bytes(head[18:20], "little") == 224:   # EM_AMDGPU: already a code object
        yield so
        return
    tmp = tempfile.mkdtemp()
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", so, os.devnull], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    for i, s in enumerate(starts):
        b, e = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.elf")
        open(b, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={b}", f"--output={e}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True)
        if r.returncode == 0 and os.path.getsize(e) > 0:
            yield e


def functions(elf):
    """(symbol, body text) of every function of one code object."""
    d = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", elf], capture_output=True, text=True).stdout
    heads = list(re.finditer(r"\n[0-9a-f]+ <([^>]+)>:\n", d))
    for i, m in enumerate(heads):
        yield m.group(1), d[m.end(): heads[i + 1].start() if i + 1 < len(heads) else len(d)]


# ---------------------------------------------------------------------------
# compare mode

META = {"vgpr": ".vgpr_count", "sgpr_spill": ".sgpr_spill_count", "lds_bytes": ".group_segment_fixed_size",
        "scratch": ".private_segment_fixed_size"}
CLASSES = ("mem", "dma", "lds", "atomic", "wait", "barrier")
MUST_EQUAL = ("lds_bytes", "mem", "dma", "atomic")


def op_class(op):
    if "atomic" in op or re.match(r"ds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)", op):
        return "atomic"
    if re.match(r"(global|buffer)_load_lds", op):
        return "dma"
    if re.match(r"(global|flat|buffer|scratch)_", op):
        return "mem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_barrier"):
        return "barrier"
    return None


def parse_kernel_meta(notes):
    """{kernel name: {field: int}} from `llvm-readelf --notes` output: the
    items of the amdhsa.kernels list, each a block of `.key: value` lines one
    level below the item's dash. Fails if the list or a field is missing."""
    lines = notes.split("\n")
    try:
        start = next(i for i, l in enumerate(lines) if l.strip() == "amdhsa.kernels:")
    except StopIteration:
        raise SystemExit("no amdhsa.kernels list in the metadata note")
    out, cur, indent = {}, None, None
    for line in lines[start + 1:]:
        m = re.match(r"^(\s*)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            if indent is not None and line.strip() and len(line) - len(line.lstrip()) < indent:
                break   # left the list
            continue
        col = len(m.group(1))
        if indent is None:
            if not m.group(2):
                raise SystemExit("amdhsa.kernels does not start with a list item")
            indent = col
        if col < indent:
            break
        if m.group(2) and col == indent:
            cur = {}
        if col + (2 if m.group(2) else 0) != indent + 2:
            continue   # a nested list (.args)
        if m.group(3) == ".name":
            out[m.group(4).strip("'\"")] = cur
        for k, f in META.items():
            if m.group(3) == f:
                cur[k] = int(m.group(4))
    for name, rec in out.items():
        missing = [f for k, f in META.items() if k not in rec]
        if missing:
            raise SystemExit(f"metadata of {name} lacks {', '.join(missing)}")
    if not out:
        raise SystemExit("no kernel in the metadata note")
    return out


def kernel_meta(elf):
    return parse_kernel_meta(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", elf], capture_output=True,
                                            text=True).stdout)


def count_classes(ins):
    """Instruction-class counts of one instruction stream (mnemonic first)."""
    c = Counter(k for k in (op_class(l.split(" ")[0]) for l in ins) if k)
    return {k: c.get(k, 0) for k in CLASSES}


def library_kernels(path):
    """{kernel name: record} over every code object of a build. A record holds
    the instruction stream (addresses and comments dropped; branch targets are
    relative, so identical code gives identical text) and the figures above."""
    out = {}
    for elf in code_objects(path):
        meta = kernel_meta(elf)
        for name, body in functions(elf):
            if name not in meta:
                continue
            ins = [re.sub(r"\s+", " ", l.split("//")[0]).strip() for l in body.split("\n")]
            ins = [l for l in ins if l and not l.endswith(":")]
            rec = dict(meta[name], ins=ins, n=len(ins), **count_classes(ins))
            if name in out and out[name]["ins"] != ins:
                raise SystemExit(f"{path}: two different copies of {name}")
            out[name] = rec
    return out


def waves(vgpr):
    """Waves per SIMD a VGPR count allows: 512 registers per lane, allocated
    in blocks of 8, and never more than the 8 wave slots of a SIMD."""
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def refusal(x, y, touched):
    """Why head record y of a kernel that differs from parent record x is not
    acceptable: a list of reasons, empty if it is."""
    why = []
    if not touched:
        why.append("control kernel differs")
    if y["scratch"] != 0:
        why.append("scratch")
    why += [k for k in MUST_EQUAL if x[k] != y[k]]
    if waves(x["vgpr"]) != waves(y["vgpr"]):
        why.append("waves/SIMD")
    return why


def compare(parent, head, md):
    a, b = library_kernels(parent), library_kernels(head)
    names = sorted(set(a) | set(b))
    dem = {nm: nm for nm in names}
    if shutil.which("c++filt"):
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        dem = dict(zip(names, out))
    fam = {}   # family -> [identical, accepted, refused]
    rows, bad = [], []
    for nm in names:
        m = re.match(r"_ZN3nbx(\d+)", nm)   # the kernel template's own name, from its length prefix
        f = nm[m.end(): m.end() + int(m.group(1))] if m else nm
        touched = f.startswith("kReduce") or f.startswith("kWide")
        tally = fam.setdefault(f, [0, 0, 0])
        if nm not in a or nm not in b:
            tally[2] += 1
            bad.append(f"{dem[nm]}: only in {'parent' if nm in a else 'head'}")
            continue
        x, y = a[nm], b[nm]
        if x["ins"] == y["ins"] and all(x[k] == y[k] for k in META):
            tally[0] += 1
            continue
        why = refusal(x, y, touched)
        tally[2 if why else 1] += 1
        if why:
            bad.append(f"{dem[nm]}: {', '.join(why)}")
        short = re.sub(r"^void nbx::", "", dem[nm]).replace("nbx::", "").split("(")[0]
        cells = [f"{x[k]} → {y[k]}" if x[k] != y[k] else str(x[k]) for k in ("n", *META, *CLASSES)]
        rows.append(f"| `{short}` | " + " | ".join(cells) + f" | {'refused: ' + ', '.join(why) if why else 'accepted'} |")
    lines = [f"{len(names)} kernels compared.", "", "| family | identical | listed, accepted | refused |", "|---|---|---|---|"]
    lines += [f"| {f} | {t[0]} | {t[1]} | {t[2]} |" for f, t in sorted(fam.items())]
    if rows:
        lines += ["", "| kernel | instructions | VGPRs | SGPR spills | LDS B | scratch B | " + " | ".join(CLASSES) + " | verdict |",
                  "|---|" + "---|" * (3 + len(META) + len(CLASSES) - 1)]
        lines += rows
    if bad:
        lines += ["", "Refused:", ""] + [f"- {x}" for x in bad]
    text = "\n".join(lines) + "\n"
    if md:
        open(md, "w").write(text)
    if len(rows) > 40:   # the table goes to --md only
        text = "\n".join(lines[:4 + len(fam)] + (lines[-(len(bad) + 3):] if bad else [])) + "\n"
    sys.stdout.write(text)
    return 1 if bad else 0


def main():
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
        return compare(sys.argv[i + 1], sys.argv[i + 2], md)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    so = os.path.join(ROOT, "neuronabox-nccl_amd", "lib", "libnbxccl.so")
    if "--so" in sys.argv:
        so = sys.argv[sys.argv.index("--so") + 1]
        args = [a for a in args if a != so]
    name = args[0]
    for e in code_objects(so):
        for sym, body in functions(e):
            if sym == name or name in sym:
                ops = re.findall(r"^\s+([a-z_0-9]+)", body, re.M)
                print(f"# {sym}: {len(ops)} instructions")
                if "--hist" in sys.argv:
                    for op, c in Counter(ops).most_common(25):
                        print(f"{c:6d} {op}")
                else:
                    print(body)
                return 0
    print("kernel not found", file=sys.stderr)
    return 1


if __name__ == "__main__":
    sys.exit(main())

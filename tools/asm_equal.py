"""Do two builds of csrc/*.hip give the same gfx950 machine code?  The proof a refactor of a kernel file rests on.

    hipcc <build_ext.FLAGS> -I include -I csrc --cuda-device-only -S -o OLD/<file>.s <file>     (at the old commit)
    ... the same into NEW/ at the new tree, then
    python tools/asm_equal.py OLD NEW

Per function: the instruction stream with comments dropped and local labels renumbered in order of appearance; per kernel: the
.amdhsa_kernel block and the code object's metadata entry (registers, LDS, scratch, kernarg size, workgroup size, arguments).
The __hip_cuid_* symbol is outside both.  K23's kernels had ten template parameters up to commit fc20909 (C, ACT, HAS_LN and
seven that were functions of C or constant); their symbols are mapped to the three-parameter ones.  Exit status 1 on any
difference."""
import glob
import os
import re
import sys

K23_OLD = re.compile(r"(mlp_split_kernelILi\d+ELi\d+ELb[01]E)(?:Li\d+E){7}E")


def units(path):
    text = K23_OLD.sub(r"\1E", open(path).read())
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        labels = {}
        lines = [ln.split(";")[0].rstrip() for ln in m.group(2).splitlines()]
        body = "\n".join(ln for ln in lines if ln.strip())
        body = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), body)
        out["code " + m.group(1)] = body
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        out["descriptor " + m.group(1)] = m.group(2)
    for m in re.finditer(r"^  - \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S | re.M):
        out["metadata " + re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)] = m.group(0)
    return out


def main(old_dir, new_dir):
    bad = total = kernels = 0
    names = sorted({os.path.basename(p) for d in (old_dir, new_dir) for p in glob.glob(os.path.join(d, "*.s"))})
    for name in names:
        a, b = (units(os.path.join(d, name)) if os.path.exists(os.path.join(d, name)) else None for d in (old_dir, new_dir))
        if a is None or b is None:
            print(f"{name}: only in {'new' if a is None else 'old'}")
            bad += 1
            continue
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        nk = sum(1 for k in b if k.startswith("metadata "))
        total += len(set(a) | set(b))
        kernels += nk
        bad += len(diff)
        print(f"{name}: {nk} kernels, {len(b)} units, {'equal' if not diff else 'DIFFERENT: ' + ', '.join(diff[:6])}")
    print(f"{len(names)} files, {kernels} kernels, {total} units compared, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

#!/usr/bin/env python3
"""Compare the kernels of two sets of `hipcc -S --cuda-device-only` listings (no GPU needed): the method of profiles/sampler_stream.md
section 1, used again for profiles/sampler_top_p.md and profiles/sampler_split.md.  The listings may come from differently named source
files: a kernel is matched by its name, wherever it was compiled.

For every kernel of the NEW listings whose demangled name matches the pattern: instructions, vector loads, VGPRs, SGPRs, scratch bytes;
and, where the OLD listings have the kernel with the same leading template arguments (the new one may carry more, e.g. a trailing
`false`), whether the body (label to .amdhsa_kernel) and the descriptor are identical once the mangled name, the function number inside
the local labels and the trailing `;` comments are taken out.  The last line counts the kernels: compared, different, new, and in OLD only.

usage: tools/sampler_isa_diff.py old.s[,old2.s...] new.s[,new2.s...] [pattern]
pattern: a glob over the demangled name, default `sample_*kernel*` (the sampler's); `*` compares every kernel.
"""
import fnmatch
import re
import shutil
import subprocess
import sys


def normalise(text, name):
    """Function numbers differ whenever a kernel's place in its module does (.LBB25_134 -> .LBBN_134), and the padding before a trailing
    comment moves with the label's width."""
    text = re.sub(r"\b(LBB|Lfunc_end|Ltmp)\d+", r"\1N", text.replace(name, "NAME"))
    return "\n".join(re.sub(r"\s*;.*$", "", l) for l in text.split("\n"))


def kernels(paths):
    out = {}
    for path in paths.split(","):
        text = open(path).read()
        for d in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
            name, desc = d.groups()
            start = re.search(r"^%s:[^\n]*\n" % re.escape(name), text, re.M).end()
            body = text[start:d.start()]
            after = text[d.end():d.end() + 4000]
            meta = {k: int(v) for k, v in re.findall(r"^; (NumVgprs|TotalNumSgprs|ScratchSize): (\d+)", after, re.M)[:3]}
            ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((";", "."))]
            out[name] = dict(body=normalise(body, name), desc=normalise(desc, name), n=len(ins),
                             loads=sum(1 for i in ins if i.startswith("global_load")), **meta)
    return out


def demangle(names):
    r = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return {n: re.sub(r"\(.*$", "", d).replace("void ", "") for n, d in zip(names, r.stdout.split("\n"))}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pattern = sys.argv[3] if len(sys.argv) > 3 else "sample_*kernel*"
    dn = demangle(list(old) + list(new))
    old, new = ({n: k for n, k in ks.items() if fnmatch.fnmatchcase(dn[n], pattern)} for ks in (old, new))

    def targs(n):
        m = re.search(r"<(.*)>", dn[n])
        return [a.strip() for a in m.group(1).split(",")] if m else []
    base = lambda n: dn[n].split("<")[0]
    print("| kernel | instructions | vector loads | VGPRs | SGPRs | scratch bytes | body vs old | descriptor vs old |")
    print("|---|---|---|---|---|---|---|---|")
    different, fresh, seen = 0, 0, set()
    for n, k in new.items():
        match = [o for o in old if base(o) == base(n) and targs(n)[:len(targs(o))] == targs(o) and all(a == "false" for a in targs(n)[len(targs(o)):])]
        if match:
            o = old[match[0]]
            seen.add(match[0])
            cmp = ("identical" if o["body"] == k["body"] else "DIFFERENT", "identical" if o["desc"] == k["desc"] else "DIFFERENT")
            different += "DIFFERENT" in cmp
        else:
            cmp = ("new", "new")
            fresh += 1
        print(f"| `{dn[n]}` | {k['n']} | {k['loads']} | {k.get('NumVgprs')} | {k.get('TotalNumSgprs')} | {k.get('ScratchSize')} | {cmp[0]} | {cmp[1]} |")
    gone = [dn[o] for o in old if o not in seen]
    print(f"\n{len(new)} kernels, {len(new) - fresh} compared with old: {different} different, {fresh} new, {len(gone)} in old only"
          + "".join(f"\n  old only: `{g}`" for g in gone))


if __name__ == "__main__":
    main()

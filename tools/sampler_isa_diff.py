#!/usr/bin/env python3
"""Compare the sampler kernels of two `hipcc -S --cuda-device-only` listings of csrc/optim_misc.hip (no GPU needed): the method of
profiles/sampler_stream.md section 1, used again for profiles/sampler_top_p.md.

For every sample_kernel / sample_wide_kernel instantiation of the NEW listing: instructions, vector loads, VGPRs, SGPRs, scratch bytes;
and, where the OLD listing has the instantiation with the same leading template arguments (the new one may carry more, e.g. a trailing
`false`), whether the body (label to .amdhsa_kernel) and the descriptor are identical once the mangled name and the function number
inside the local labels are replaced.

usage: tools/sampler_isa_diff.py old.s new.s
"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w*(?:sample_kernel|sample_wide_kernel)\w*):[^\n]*\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        name, body, desc = m.groups()
        fn = re.search(r"\.LBB(\d+)_", body)
        norm = lambda s: re.sub(r"(LBB|Lfunc_end|Ltmp)%s\b" % (fn.group(1) if fn else "X"), r"\1N", s).replace(name, "NAME")
        after = text[m.end():m.end() + 4000]
        meta = {k: int(v) for k, v in re.findall(r"^; (NumVgprs|TotalNumSgprs|ScratchSize): (\d+)", after, re.M)[:3]}
        ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((";", "."))]
        out[name] = dict(body=norm(body), desc=norm(desc), n=len(ins), loads=sum(1 for i in ins if i.startswith("global_load")), **meta)
    return out


def demangle(names):
    import shutil
    r = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return {n: re.sub(r"\(.*$", "", d).replace("void ", "") for n, d in zip(names, r.stdout.split("\n"))}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    dn = demangle(list(old) + list(new))
    targs = lambda n: [a.strip() for a in re.search(r"<(.*)>", dn[n]).group(1).split(",")]
    base = lambda n: dn[n].split("<")[0]
    print("| instantiation | instructions | vector loads | VGPRs | SGPRs | scratch bytes | body vs old | descriptor vs old |")
    print("|---|---|---|---|---|---|---|---|")
    for n, k in new.items():
        match = [o for o in old if base(o) == base(n) and targs(n)[:len(targs(o))] == targs(o) and all(a == "false" for a in targs(n)[len(targs(o)):])]
        if match:
            o = old[match[0]]
            cmp = ("identical" if o["body"] == k["body"] else "DIFFERENT", "identical" if o["desc"] == k["desc"] else "DIFFERENT")
        else:
            cmp = ("new", "new")
        print(f"| `{dn[n]}` | {k['n']} | {k['loads']} | {k.get('NumVgprs')} | {k.get('TotalNumSgprs')} | {k.get('ScratchSize')} | {cmp[0]} | {cmp[1]} |")


if __name__ == "__main__":
    main()

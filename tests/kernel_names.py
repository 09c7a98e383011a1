"""Kernel names as a kernel trace reports them, for the host tests of the plan headers (test_ffmid_plan_host.py, test_norm_plan_host.py)."""
import re


def parse_kernel(name):
    """(copy namespace, kernel, template arguments) of a kernel name as the trace has it -- demangled, or Itanium-mangled where the
    demangler does not know the 16-bit types; types as h16 / float, numbers and flags as ints"""
    m = re.match(r"(?:void )?(omlm_\w+)::(\w+)(?:<([^>]*)>)?\(", name)
    if m:
        if "_Accum" in (m.group(3) or ""):
            return m.group(1), m.group(2), _mangled_args(_remangle(m.group(3)), name)
        args = m.group(3) or ""
        words = {"true": 1, "false": 0, "float": "float", "__bf16": "h16", "_Float16": "h16"}
        return m.group(1), m.group(2), [words[a] if a in words else int(a) for a in args.split(", ")] if args else []
    m = re.match(r"_ZN(\d+)", name)
    assert m, name
    at = 3 + len(m.group(1))
    ns, at = name[at:at + int(m.group(1))], at + int(m.group(1))
    m = re.match(r"(\d+)", name[at:])
    at += len(m.group(1))
    kernel, rest = name[at:at + int(m.group(1))], name[at + int(m.group(1)):]
    m = re.match(r"I((?:Li\d+E|Lb[01]E|DF16_|DF16b|f)+)E", rest)
    assert m, name
    return ns, kernel, _mangled_args(m.group(1), name)


def _mangled_args(text, name):
    """template arguments in their Itanium mangling: types (f, DF16_, DF16b) and literals (Li<n>E, Lb<0|1>E)"""
    assert re.fullmatch(r"(?:Li\d+E|Lb[01]E|DF16_|DF16b|f)+", text), (name, text)
    return [int(t[2:-1]) if t[0] == "L" else "float" if t == "f" else "h16" for t in re.findall(r"Li\d+E|Lb[01]E|DF16_|DF16b|f", text)]


def _remangle(args):
    """The profiler's demangler reads the bf16 type (DF16b) as a fixed-point type and swallows the `L` of a literal behind it; the literal's
    type then stands alone and its digits are read as the length of a name: `DF16bLi2ELb1E` comes out as "bool _Accum, int, EL, bool, E",
    `DF16bLb1ELb0E` as "bool _Accum, bool, E, false".  (Where the literal's value is 0 the name stays mangled.)  Nothing is lost: every
    token goes back to the characters it was read from."""
    back = {"bool _Accum": "DF16bL", "int": "i", "bool": "b", "float": "f", "true": "Lb1E", "false": "Lb0E", "_Float16": "DF16_", "__bf16": "DF16b"}
    return "".join(back[t] if t in back else f"Li{t}E" if re.fullmatch(r"-?\d+", t) else f"{len(t)}{t}" for t in args.split(", "))

"""include/fgo.h read as text (test infrastructure): the functions it declares, for the tests that hold the ctypes binding to it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fgo.h")


def _strip_braces(src):
    """the text with every {...} body (the typedef'd structs, and the extern "C" block's own braces) taken out"""
    out, depth = [], 0
    for ch in src:
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif depth == 0:
            out.append(ch)
    return "".join(out)


def _type_of(param):
    """the type of one parameter, its name dropped and spacing normalised: 'const double *info_ut21' -> 'const double *',
    'double out[36]' -> 'double *'"""
    p = " ".join(param.split())
    m = re.match(r"^(.*?)(\b\w+)?\s*(\[\s*\d*\s*\])?$", p)
    base, name, arr = m.group(1).strip(), m.group(2), m.group(3)
    if not base:                                    # a bare type such as 'void' or 'int': the "name" was the type
        base, name = name, None
    base = base.replace(" *", "*").replace("* ", "*").replace("*", " *")
    return base + (" *" if arr else "")


def declared_functions():
    """[(return type, name, [parameter types])] for every function include/fgo.h declares, in its order"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)
    src = re.sub(r'extern\s+"C"\s*\{', "", src)     # its closing brace sits under an #ifdef and goes with the depth count below
    src = _strip_braces(src)
    out = []
    for stmt in src.split(";"):
        s = " ".join(stmt.split())
        if not s or s.startswith("typedef"):
            continue
        m = re.match(r"^(?:FGO_API\s+)?(.+?)\b(fgo_\w+)\s*\((.*)\)$", s)
        if not m:
            continue
        ret = m.group(1).strip().replace(" *", "*").replace("*", " *")
        args = m.group(3).strip()
        params = [] if args in ("", "void") else [_type_of(a) for a in args.split(",")]
        out.append((ret, m.group(2), params))
    return out

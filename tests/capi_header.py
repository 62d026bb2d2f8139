"""The prototypes of include/rvb_capi.h as data: what tests/test_capi_calls_host.py canonicalises a call's arguments by and what
tests/test_capi_host.py holds capi.py's signature table against.  Comments are stripped and prototypes spanning lines are joined."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rvb_capi.h")

# parameter / return classes, and the ctypes type a table entry of that class must be
CLASSES = {"pointer": ctypes.c_void_p, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "void": None, "const char *": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s*\*)?)\s*\b(rvb_\w+)\s*\(([^()]*)\)\s*(?=;)")


def _class(declaration, is_return=False):
    d = " ".join(declaration.replace("*", " * ").split())
    if is_return and d == "const char *":
        return "const char *"
    if "*" in d or "[" in d:
        return "pointer"
    words = [w for w in d.split() if w != "const"]
    kind = words[0]                                  # the parameter's name, when there is one, follows the type
    assert kind in CLASSES and kind != "void" or (is_return and kind == "void"), declaration
    return kind


def prototypes(path=HEADER):
    """[(name, return class, [parameter class, ...]), ...] in the header's order."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    out = []
    for ret, name, params in _PROTOTYPE.findall(" ".join(text.split())):
        params = [p for p in params.split(",") if p.strip() and p.strip() != "void"]
        out.append((name, _class(ret, True), [_class(p) for p in params]))
    return out

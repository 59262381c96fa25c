"""The binding's ABI table against the headers, for every export at once (host only).

Three nets under the ctypes binding of libstego_corr.so:
  * signatures: every name of capi.SIGNATURES is declared in exactly one header of include/, exported by the loaded library, and
    its return type, argument count and every argument's ctypes type are what the header's C declaration says; every declaration of
    the headers is bound.  No exemption list.
  * layouts: a generated C program, compiled against include/, prints sizeof and every offsetof of every ctypes.Structure the
    binding defines (field names from _fields_: a field the header lacks does not compile); all agree with ctypes.
  * constants: every X_ERR_Y of the binding is STEGO_ERR_X_Y of a header, and every other upper-case integer NAME with a
    `#define STEGO_NAME` or an enum member `STEGO_NAME = value` has that value.
"""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from stego_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32,
           "uint8_t": ctypes.c_uint8}


def _headers():
    """{header file name: its text without comments}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(INCLUDE, "*.h"))):
        with open(path) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        out[os.path.basename(path)] = re.sub(r"//[^\n]*", " ", text)
    return out


def _param(text):
    """One C parameter -> (base type name, pointer depth); `T name[...]` counts as a pointer."""
    depth = text.count("*") + (1 if "[" in text else 0)
    words = re.sub(r"\[[^\]]*\]", " ", text.replace("*", " ")).split()
    words = [w for w in words if w not in ("const", "struct")]
    assert words, text
    # a scalar or pointer parameter is `type name`; the headers name every parameter
    assert len(words) == 2, "cannot read the parameter %r" % text
    return words[0], depth


def _declarations():
    """{export: [(header, return (base, depth), [(base, depth) per parameter])]} of every `stego_*(` of the headers."""
    decls = {}
    for header, text in _headers().items():
        code = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
        found = set()
        for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(stego_\w+)\s*\(([^()]*)\)\s*;", code):
            ret, name, params = m.group(1), m.group(2), m.group(3).strip()
            rwords = [w for w in ret.replace("*", " ").split() if w not in ("const", "extern")]
            assert len(rwords) == 1, "cannot read the return type %r of %s" % (ret, name)
            args = [] if params in ("", "void") else [_param(p) for p in params.split(",")]
            decls.setdefault(name, []).append((header, (rwords[0], ret.count("*")), args))
            found.add(name)
        # every `stego_name(` left in the code of the header is one of the declarations just read
        for name in re.findall(r"\b(stego_\w+)\s*\(", code):
            assert name in found, "%s: `%s(` is not a declaration this test can read" % (header, name)
    return decls


def _is_pointer_to(ctype, target):
    return isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer) and ctype._type_ is target


def _arg_agrees(ctype, base, depth):
    if depth == 0:
        if base == "stego_stream_t":
            return ctype is ctypes.c_void_p
        return base in SCALARS and ctype is SCALARS[base]
    if depth >= 2:
        return ctype is ctypes.c_void_p or _is_pointer_to(ctype, ctypes.c_void_p)
    if ctype is ctypes.c_void_p:
        return True
    if base.startswith("Stego"):
        struct = getattr(capi, base, None)
        return struct is not None and _is_pointer_to(ctype, struct)
    return base in SCALARS and _is_pointer_to(ctype, SCALARS[base])


def _ret_agrees(ctype, base, depth):
    if depth == 0:
        return base in SCALARS and ctype is SCALARS[base]
    if base == "char":
        return ctype is ctypes.c_char_p
    return ctype is ctypes.c_void_p


def test_every_signature_is_the_headers_declaration():
    decls = _declarations()
    lib = capi.load()
    assert len(capi.SIGNATURES) >= 115
    problems = []
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        found = decls.get(name, [])
        if len(found) != 1:
            problems.append("%s: declared in %s (exactly one header expected)" % (name, [h for h, _, _ in found]))
            continue
        header, ret, args = found[0]
        if not hasattr(lib, name):
            problems.append("%s: not exported by the library" % name)
        if not _ret_agrees(restype, *ret):
            problems.append("%s: returns %s in %s, %s in the binding" % (name, ret, header, restype))
        if len(args) != len(argtypes):
            problems.append("%s: %d arguments in %s, %d in the binding" % (name, len(args), header, len(argtypes)))
            continue
        for i, (ctype, (base, depth)) in enumerate(zip(argtypes, args)):
            if not _arg_agrees(ctype, base, depth):
                problems.append("%s: argument %d is %s%s in %s, %s in the binding" % (name, i, base, "*" * depth, header, ctype))
    assert not problems, "\n".join(problems)


def test_every_header_declaration_is_bound():
    unbound = sorted(set(_declarations()) - set(capi.SIGNATURES))
    assert not unbound, "declared in include/ but not in capi.SIGNATURES: %s" % unbound


def _structures():
    return sorted((v for v in vars(capi).values()
                   if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure),
                  key=lambda c: c.__name__)


def test_struct_layouts_are_the_headers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler (cc / gcc) to compile the layout program with")
    structs = _structures()
    assert len(structs) >= 31
    lines = ["#include <stdio.h>", "#include <stddef.h>"]
    lines += ['#include "%s"' % h for h in sorted(_headers())]
    lines.append("int main(void) {")
    for s in structs:
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (s.__name__, s.__name__))
        for field in s._fields_:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s.__name__, field[0], s.__name__, field[0]))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layouts.c", tmp_path / "layouts"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-I", INCLUDE, "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        struct, what, value = line.split()
        got[(struct, what)] = int(value)
    want = {}
    for s in structs:
        want[(s.__name__, "sizeof")] = ctypes.sizeof(s)
        for field in s._fields_:
            want[(s.__name__, field[0])] = getattr(s, field[0]).offset
    assert got == want, sorted(set(got.items()) ^ set(want.items()))


def _header_constants():
    """({STEGO_ERR_X: value} of the enums, {STEGO_NAME: value} of the #defines and of the other enum members `STEGO_NAME = value`
    that evaluate to an integer)"""
    errs, values = {}, {}
    for text in _headers().values():
        found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(STEGO_\w+)[ \t]+(.+?)[ \t]*$", text, flags=re.M)
        found += re.findall(r"\b(STEGO_\w+)\s*=\s*([^,}=]+?)\s*[,}]", text)
        for name, value in found:
            if re.fullmatch(r"[\d\s()<+\-*xXa-fA-FuUlL]+", value):
                number = int(eval(re.sub(r"(?<=[\da-fA-F])[uUlL]+\b", "", value), {"__builtins__": {}}))
                (errs if name.startswith("STEGO_ERR_") else values)[name] = number
    return errs, values


def _binding_constants():
    return {n: v for n, v in vars(capi).items() if n.isupper() and type(v) is int}


def test_error_codes_are_the_headers():
    errs, _ = _header_constants()
    mine = {n: v for n, v in _binding_constants().items() if "_ERR_" in n}
    assert len(mine) >= 76      # (what the binding held when this test was written: the parser still finds them)
    for name, value in mine.items():
        unit, code = name.split("_ERR_", 1)
        assert errs.get("STEGO_ERR_%s_%s" % (unit, code)) == value, name


def test_constants_the_headers_define_have_their_value():
    _, defines = _header_constants()
    checked = 0
    for name, value in _binding_constants().items():
        if "_ERR_" in name or "STEGO_" + name not in defines:
            continue
        assert defines["STEGO_" + name] == value, name
        checked += 1
    assert checked >= 117

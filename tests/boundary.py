"""The checks every binding of a public header is held to, written once (tests/test_nnscore_cpu.py, test_refine_cpu.py and
test_plane_cpu.py call them with their header, module and names; tests/test_abi.py reads its prototypes here): the header's
prototypes against the module's SIGNATURES and the library's exports, and the module's STRUCTS against gcc's layout of the
header's structs."""
import ctypes
import re
import subprocess


def stripped(header):
    """The header's text without comments and preprocessor lines."""
    src = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return re.sub(r"^\s*#.*$", " ", src, flags=re.M)


def prototypes(header):
    """{name: (return type, [parameter types])} of every `ret vcr_name(params);` of a header, comments and preprocessor lines
    stripped; a type is its base name with one '*' per level of indirection, `const` and parameter names dropped."""
    def ctype(text, named):
        tok = text.replace("*", " * ").split()
        if named and len(tok) >= 2 and tok[-1] != "*":       # a type is one word or ends in '*': what follows is the name
            tok = tok[:-1]
        tok = [t for t in tok if t != "const"]
        assert len(tok) >= 1 and all(t == "*" for t in tok[1:]), text
        return tok[0] + "*" * (len(tok) - 1)
    out = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\**)\s*\b(vcr_\w+)\s*\(([^()]*)\)\s*;", stripped(header)):
        assert name not in out, name
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (ctype(ret, False), [ctype(p, True) for p in params])
    return out


def check_signatures(header, module, lib, names):
    """The header declares exactly `names`, and so does module.SIGNATURES; per prototype the arity, the return type, every
    scalar exactly, every struct pointer as POINTER of the mirror module.STRUCTS names, every other pointer (and vcr_stream_t)
    as some pointer-typed parameter; the library exports the name, and `lib` (the module's typed one) carries the table."""
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "float": ctypes.c_float}
    protos = prototypes(header)
    assert set(protos) == set(module.SIGNATURES) == set(names)
    for name, (ret, params) in protos.items():
        res, args = module.SIGNATURES[name]
        assert res is scalars[ret], (name, ret, res)
        assert len(args) == len(params), (name, params, args)
        for i, (c, t) in enumerate(zip(params, args)):
            if c in scalars:
                assert t is scalars[c], (name, i, c, t)
            elif c.startswith("vcr_") and c != "vcr_stream_t":
                assert c.endswith("*") and not c.endswith("**"), (name, i, c)
                assert t is ctypes.POINTER(module.STRUCTS[c[:-1]]), (name, i, c, t)
            else:
                assert c == "vcr_stream_t" or c.endswith("*"), (name, i, c)
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, i, c, t)
        assert hasattr(lib, name), f"{name} declared in {header} but not exported"
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def check_layout(header, module, tmp_path):
    """sizeof and the offset of every field of each struct of module.STRUCTS, as gcc lays out the header, against the ctypes
    mirror; and a fresh mirror says its own size in struct_bytes."""
    hdr = stripped(header)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void) {']
    expect = []
    for cname, ct in module.STRUCTS.items():
        assert re.search(r"typedef struct[^{]*\{[^{}]*\}\s*%s;" % cname, hdr), cname
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append((cname, "sizeof", ctypes.sizeof(ct)))
        for fname, _ in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append((cname, fname, getattr(ct, fname).offset))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [e for _, _, e in expect], list(zip(expect, got))
    for ct in module.STRUCTS.values():
        assert ct().struct_bytes == ctypes.sizeof(ct)

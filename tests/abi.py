"""The C ABI as include/acgan_hip.h declares it, parsed once (standard library only): every entry point's return and
argument kinds, every struct's fields, the version.  A kind is 'ptr' (any pointee), 'int', 'size_t', 'long long', 'float' or
'double'; `kind_of` maps a ctypes type onto the same words, so a binding is compared with the header position by position."""
import ctypes
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "acgan_hip.h")
SCALARS = ("long long", "size_t", "double", "float", "int")


@functools.lru_cache(maxsize=None)
def source():
    """the header without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return re.sub(r"(?m)^\s*#.*$", " ", re.sub(r"//[^\n]*", " ", text))


@functools.lru_cache(maxsize=None)
def defines():
    return {k: int(v) for k, v in re.findall(r"(?m)^#define\s+(ACG_\w+)\s+(-?\d+)\s*$", open(HEADER).read())}


def header_version():
    return defines()["ACG_VERSION"]


def _kind(ctype):
    """'const float *' -> 'ptr', 'unsigned' -> refused: the ABI passes only the six kinds"""
    if "*" in ctype:
        return "ptr"
    words = " ".join(w for w in ctype.split() if w != "const")
    assert words in SCALARS, ctype
    return words


def _declarator(base, decl):
    """('const float', '*w[4]') -> ('w', 'ptr', 4); array lengths may be ACG_* defines"""
    m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", decl)
    assert m, (base, decl)
    n = m.group(3)
    return m.group(2), _kind(base + m.group(1)), (None if n is None else defines()[n] if n in defines() else int(n))


@functools.lru_cache(maxsize=None)
def structs():
    """struct name -> [(field, kind, array length or None)], in order; `const float *w[4], *b[4];` gives two fields"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", source()):
        fields = []
        for line in filter(None, (s.strip() for s in body.split(";"))):
            base, first = re.fullmatch(r"((?:const\s+)?(?:long\s+long|\w+))\s*(.*)", line, flags=re.S).groups()
            fields += [_declarator(base, d) for d in first.split(",")]
        out[name] = fields
    return out


@functools.lru_cache(maxsize=None)
def declarations():
    """entry point -> (return kind, [argument kinds])"""
    text = re.sub(r"typedef\s+(?:struct|enum)\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", source())
    out = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(acg_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [a.strip() for a in args.split(",")]
        # an argument is `type name`: the kind is what stands before the name, the stars included
        out[name] = (_kind(ret), [] if args == ["void"] else [_kind(re.fullmatch(r"(.*?)\w+", a, flags=re.S).group(1)) for a in args])
    return out


def header_args(name):
    """the argument kinds of one entry point"""
    return declarations()[name][1]


def kind_of(ctype):
    """the header's word for a ctypes type"""
    if ctype is ctypes.c_void_p or ctype is ctypes.c_char_p or isinstance(ctype, type(ctypes.POINTER(ctypes.c_int))):
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_size_t: "size_t", ctypes.c_longlong: "long long", ctypes.c_float: "float",
            ctypes.c_double: "double"}[ctype]


def structure_fields(cls):
    """a ctypes.Structure's fields in the shape of structs()"""
    return [(k, kind_of(t._type_), t._length_) if issubclass(t, ctypes.Array) else (k, kind_of(t), None) for k, t in cls._fields_]

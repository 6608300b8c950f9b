"""Both sides of the Python <-> C boundary in one shape, for tests/test_abi_cpu.py.

``header()`` is what a C++ compiler sees in include/selfmask_hip.h: ONE generated program, compiled and run once per test session,
prints every struct's size and alignment, every field's offset, kind and element count, every prototype's return and parameter
kinds and every SM_* macro's value.  ``mirror()`` is the same dict read off the ctypes definitions of selfmask_amd/_native.py.
``header_structs()`` / ``header_macros()`` parse the header's text for what no compiler can be asked: the names.

Kind codes: p = any pointer, iN / uN = integer of N bytes by signedness, fN = float of N bytes, c1 = char, sN = a nested struct of
N bytes, v = a void return."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

from selfmask_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "selfmask_hip.h")

_PRELUDE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "%s"
template <class T> void kind() {
    if (std::is_pointer<T>::value) printf(" p");
    else if (std::is_same<T, char>::value) printf(" c1");
    else if (std::is_floating_point<T>::value) printf(" f%%zu", sizeof(T));
    else if (std::is_integral<T>::value) printf(" %%c%%zu", std::is_signed<T>::value ? 'i' : 'u', sizeof(T));
    else printf(" s%%zu", sizeof(T));
}
template <> void kind<void>() { printf(" v"); }
template <class F> struct proto;
template <class R, class... A> struct proto<R (*)(A...)> {
    static void put() { kind<R>(); int in_order[] = {0, (kind<A>(), 0)...}; (void)in_order; }
};
#define STRUCT(T) printf("S " #T " %%zu %%zu\n", sizeof(T), alignof(T))
#define FIELD(T, f) do { typedef std::remove_all_extents<decltype(T::f)>::type E; printf("F " #T " " #f " %%zu", offsetof(T, f)); \
                         kind<E>(); printf(" %%zu\n", sizeof(T::f) / sizeof(E)); } while (0)
#define PROTO(f) do { printf("P " #f); proto<decltype(&f)>::put(); printf("\n"); } while (0)
#define MACRO(m) printf("M " #m " %%lld\n", (long long)(m))
int main() {
"""


def _text() -> str:
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def header_structs() -> dict:
    """typedef name -> field names in declaration order, from the header's text"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(sm_\w+)\s*;", _text()):
        decls = [d for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
        out[name] = [re.findall(r"[A-Za-z_]\w*", re.sub(r"\[[^\]]*\]", "", d))[-1] for d in decls]
    return out


def header_macros() -> list:
    return re.findall(r"^#define\s+(SM_\w+)\b", _text(), flags=re.M)


def compiler() -> list:
    """any host C++ compiler; the build's own hipcc is one (a clang driver, here on plain C++: no device pass)"""
    for cxx in ("g++", "c++", "clang++"):
        if shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no C++ compiler and no hipcc: the ABI mirror cannot be checked"
    return [hipcc, "-x", "c++"]


@functools.lru_cache(maxsize=None)
def header() -> dict:
    lines = [_PRELUDE % HEADER]
    for cname, ct in N.STRUCTS.items():
        lines.append(f"STRUCT({cname});")
        lines += [f"FIELD({cname}, {f});" for f, _ in ct._fields_]
    lines += [f"PROTO({name});" for name in N.SYMBOLS] + [f"MACRO({m});" for m in header_macros()] + ["return 0; }"]
    tmp = tempfile.mkdtemp(prefix="sm_abi_probe_")
    src, exe = os.path.join(tmp, "probe.cpp"), os.path.join(tmp, "probe")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    cc = subprocess.run(compiler() + ["-std=c++14", "-Wno-invalid-offsetof", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, "the mirror names something the header does not have:\n" + cc.stderr[-3000:]
    out = {"struct": {}, "field": {}, "proto": {}, "macro": {}}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        tag, name, *rest = line.split()
        if tag == "S":
            out["struct"][name] = (int(rest[0]), int(rest[1]))
        elif tag == "F":
            out["field"][name, rest[0]] = (int(rest[1]), rest[2], int(rest[3]))
        elif tag == "P":
            out["proto"][name] = rest
        else:
            out["macro"][name] = int(rest[0])
    return out


def ctypes_kind(t) -> str:
    if t is None:
        return "v"
    if issubclass(t, C.Structure):
        return f"s{C.sizeof(t)}"
    code = t._type_
    if not isinstance(code, str) or code in "PzZ":  # POINTER(..), c_void_p, c_char_p, c_wchar_p
        return "p"
    if code == "c":
        return "c1"
    if code in "fdg":
        return f"f{C.sizeof(t)}"
    return ("i" if code.islower() else "u") + str(C.sizeof(t))


def mirror() -> dict:
    """header()'s dict from the ctypes side; a macro SM_X the module has no X for is left out"""
    out = {"struct": {}, "field": {}, "proto": {}, "macro": {}}
    for cname, ct in N.STRUCTS.items():
        out["struct"][cname] = (C.sizeof(ct), C.alignment(ct))
        for f, t in ct._fields_:
            count = 1
            while issubclass(t, C.Array):
                count, t = count * t._length_, t._type_
            out["field"][cname, f] = (getattr(ct, f).offset, ctypes_kind(t), count)
    for name, (res, args) in N.SYMBOLS.items():
        out["proto"][name] = [ctypes_kind(res)] + [ctypes_kind(a) for a in args]
    out["macro"] = {m: getattr(N, m[3:]) for m in header_macros() if hasattr(N, m[3:])}
    return out

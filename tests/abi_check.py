"""What the C-ABI tests read out of the headers of include/: the structs and functions a header
declares (by regex) and, by compiling a C program with gcc, the sizes, field offsets and macro
values the ctypes mirrors in mli_nerf_amd/_lib.py are compared with (tests/test_abi.py)."""
import os
import re
import subprocess

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

STRUCT = re.compile(r"}\s*(mli_\w+)\s*;")
FUNCTION = re.compile(r"^(?:int|const char\*)\s+(mli_\w+)\s*\(", re.M)
FUNCTION_ARGS = re.compile(r"^int\s+(mli_\w+)\s*\(\s*const\s+(mli_\w+)\s*\*", re.M)


def _text(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return f.read()


def declared_structs(header):
    return set(STRUCT.findall(_text(header)))


def declared_functions(header):
    return set(FUNCTION.findall(_text(header)))


def arg_structs(header):
    """{function: C name of the struct its first argument points to}."""
    return dict(FUNCTION_ARGS.findall(_text(header)))


def gcc_layout(headers, structs, macros, tmp_path):
    """What gcc makes of ``headers``: {"<struct>": size, "<struct>.<field>": offset, "<macro>": value}
    for ``structs`` ({C name: ctypes mirror}, whose field names are looked up) and ``macros`` (names)."""
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + ['#include "%s"' % h for h in headers] + ["int main(void) {"]
    for cname, st in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for m in macros:
        lines.append('printf("%s %%.17g\\n", (double)(%s));' % (m, m))
    lines += ["return 0; }"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: float(v) for k, v in (line.split() for line in out.splitlines())}

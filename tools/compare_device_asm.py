#!/usr/bin/env python3
"""compare the device-only assembly of two builds (hipcc --cuda-device-only -S
with the Makefile's flags), file by file: usage compare_device_asm.py DIR_A DIR_B

File and line directives, comments and the per-path __hip_cuid_ symbol are
dropped.  Files that differ as text are compared function by function, with the
function number in local labels (.LBBn_m, .Lfunc_endn, ...) normalised: a
launcher that names the same instantiations in another order makes the
compiler emit the same functions in another order, numbered differently."""
import hashlib
import os
import re
import sys


def clean(text):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    out = []
    for line in text.split("\n"):
        line = line.split(";")[0].rstrip()
        if not line or re.match(r"\s*\.(file|loc|ident)\b", line):
            continue
        out.append(line)
    return out


def functions(lines):
    """{symbol: hash of its body and of its .amdhsa kernel descriptor}"""
    found, name, body = {}, None, []
    for line in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        if name:
            body.append(re.sub(r"(\.L[A-Za-z_]*?)\d+(_\d+)?\b", r"\1N\2", line))
        if name and re.match(r"\s*\.end_amdhsa_kernel|\s*\.size\s+%s," % re.escape(name), line) \
                and (line.strip().startswith(".end_amdhsa") or name not in kernels(lines)):
            found[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()
            name = None
    return found


_kernels = {}


def kernels(lines):
    key = id(lines)
    if key not in _kernels:
        _kernels[key] = {m.group(1) for line in lines
                         for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)] if m}
    return _kernels[key]


def main(a, b):
    bad = 0
    for name in sorted(os.listdir(a)):
        if not name.endswith(".s"):
            continue
        la, lb = clean(open(os.path.join(a, name)).read()), clean(open(os.path.join(b, name)).read())
        if la == lb:
            print("%-16s identical text (%d lines)" % (name, len(la)))
            continue
        fa, fb = functions(la), functions(lb)
        differ = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
        print("%-16s other order of emission; %d / %d functions, same set: %s, bodies or "
              "descriptors that differ: %d" % (name, len(fa), len(fb), set(fa) == set(fb),
                                               len(differ)))
        for k in differ:
            print("    " + k)
        bad += len(differ) + (set(fa) != set(fb))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

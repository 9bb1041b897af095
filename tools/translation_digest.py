#!/usr/bin/env python3
"""Digests of the translations (csrc/host/translate.cpp, dprog_host) of the corpus of
device_code_digest.py.  Needs no GPU.  Two trees whose outputs are equal line for line translate
every program of the corpus to the same entries, annotations, fields, errno and message: the
check a change to the translator that means to change nothing runs before and after
(device_code_digest.py sees the compiled bytes only).

One line per program: name, errno of ebpf_prog_device_info, line count and sha256 of the
translation's dump (EBPF_XLATE_DUMP, csrc/host/xlate_dump.cpp).  Map handles are heap addresses,
so every handle in the dump becomes MAP<k> before hashing; two processes then agree.

EBPF_LIB=path loads another build of the library (native.py)."""
import argparse
import ctypes
import hashlib
import os
import re
import sys
import tempfile

import device_code_digest as dcd
from generic_ebpf_amd import native


def translation(env, dump, code, relocs, specs, sem):
    """(errno, the dump with its map handles replaced) of one program"""
    maps = [native.HashMap(env, s[1], s[2], s[3]) if s[0] == "hash" else native.Map(env, s[1], s[2])
            for s in specs]
    p = native.Prog(env, native.patch_relocs(code, relocs, [m.handle for m in maps]))
    try:
        if sem:
            p.set_semantics(native.SEM_STANDARD)
        open(dump, "w").close()
        err = native.lib().ebpf_prog_device_info(p.ptr, ctypes.byref(native.DprogInfo()))
        with open(dump) as f:
            text = f.read()
        for k, m in enumerate(maps):
            text = re.sub(r"\b%s\b" % hex(m.handle), "MAP%d" % k, text)
        return err, text
    finally:
        p.destroy()
        for m in maps:
            m.destroy()


def dumps(progs):
    """yields (name, errno, dump) per program of a corpus() list"""
    env = native.Env()
    fd, dump = tempfile.mkstemp(prefix="xlate_dump_")
    os.close(fd)
    os.environ["EBPF_XLATE_DUMP"] = dump
    try:
        for name, code, relocs, specs, sem in progs:
            yield (name,) + translation(env, dump, code, relocs, specs, sem)
    finally:
        del os.environ["EBPF_XLATE_DUMP"]
        os.unlink(dump)
        assert env.destroy() == 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", default=",".join(dcd.GROUPS), help="of " + ", ".join(dcd.GROUPS))
    ap.add_argument("--seeds", type=int, default=300, help="randprog seeds (group random)")
    ap.add_argument("-o", "--output", help="file to write (default: standard output)")
    a = ap.parse_args()
    groups = [g for g in a.groups.split(",") if g]
    assert all(g in dcd.GROUPS for g in groups), groups
    os.environ.pop("EBPF_XLATE_KEEP_LOOPCNT", None)
    out = open(a.output, "w") if a.output else sys.stdout
    nprog = nerr = nlines = 0
    for name, err, text in dumps(dcd.corpus(groups, a.seeds)):
        nprog, nerr, nlines = nprog + 1, nerr + (err != 0), nlines + text.count("\n")
        out.write("%s %d %d %s\n" % (name, err, text.count("\n"), hashlib.sha256(text.encode()).hexdigest()))
    if a.output:
        out.close()
    print("%d programs, %d with an errno, %d dump lines" % (nprog, nerr, nlines), file=sys.stderr)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Digests of what the assembly generator (csrc/asm/gen_interp.py) writes: the three images'
sources and asm_handlers.h, in the default environment and under every EBPF_ASM_* build knob.
Needs no GPU and no built library.  Two trees whose outputs are equal line for line generate the
same bytes: the check a change to the generator that means to change no emitted byte runs before
and after.

The generator runs as a subprocess, through its entry point and command line, so the same tool
measures any tree's generator: its path is the argument (default: this tree's).

One line per (knob setting, output file): setting, file, length, sha256.  A setting whose three
image sources all equal the default's is unexercised: the tool fails.  --default-only runs the
default environment alone."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, "generic-ebpf_amd", "csrc", "asm", "gen_interp.py")
FILES = ("m1.s", "m0.s", "m3.s", "asm_handlers.h")
# (defaults: EBPF_ASM_RETK=8, EBPF_ASM_GENHOIST=16, EBPF_ASM_NT=3, no explicit policies)
SETTINGS = [{}] + [{"EBPF_ASM_RETK": k} for k in "124"] + [{"EBPF_ASM_GENHOIST": "0"}] + \
    [{"EBPF_ASM_NT": n} for n in "012"] + \
    [{"EBPF_ASM_LDPOL": "sc1+nt"}, {"EBPF_ASM_STPOL": "none"}, {"EBPF_ASM_PROBEPOL": "sc0"}]


def run(generator, setting):
    """[(file, length, sha256)] of one generator run under `setting`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBPF_ASM_")}
    env.update(setting)
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, f) for f in FILES]
        subprocess.run([sys.executable, generator] + paths, check=True, env=env)
        out = []
        for f, p in zip(FILES, paths):
            with open(p, "rb") as fh:
                data = fh.read()
            out.append((f, len(data), hashlib.sha256(data).hexdigest()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("generator", nargs="?", default=GENERATOR, help="path to gen_interp.py")
    ap.add_argument("--default-only", action="store_true", help="the default environment alone")
    ap.add_argument("-o", "--output", help="file to write (default: standard output)")
    a = ap.parse_args()
    out = open(a.output, "w") if a.output else sys.stdout
    default, idle = None, []
    for setting in SETTINGS[:1] if a.default_only else SETTINGS:
        res = run(a.generator, setting)
        for f, n, h in res:
            out.write("%s %s %d %s\n" % (",".join("%s=%s" % kv for kv in setting.items()) or "-", f, n, h))
        if default is None:
            default = res
        elif res[:3] == default[:3]:
            idle.append(setting)
    if a.output:
        out.close()
    if idle:
        sys.exit("knobs that change no image: %s" % idle)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One line per device function of the library: "<source> <symbol> <sha256 of its body>", sorted.

Every kernels source is compiled to gfx950 assembly with the flags tests/test_operand_rule_cpu.py uses
(-S --cuda-device-only).  A body is the text from the symbol's label to its .Lfunc_end label, the kernel descriptor
included, with comments stripped and the function index taken out of the local labels (.LBB<n>_ -> .LBB_): moving a
host function reorders the device functions of a file and changes nothing else.  Two trees hold the same device code
when their listings are equal.

    python tools/device_code_digest.py [-j JOBS] [--summary] [csrc directory] > listing.txt

--summary prints one line per source instead: "<source> <functions> <sha256 of its lines of the listing>".
"""
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = "/opt/rocm/bin/hipcc"
TYPE = re.compile(r"^\s+\.type\s+(\S+),@function")
END = re.compile(r"^\.Lfunc_end\d+:")
NUMBERED = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+")


def functions(asm):
    """(symbol, sha256) of every function in an assembly text"""
    name, body = None, None
    for line in asm.splitlines():
        m = TYPE.match(line)
        if m:
            name, body = m.group(1), []
        elif name and END.match(line):
            yield name, hashlib.sha256("\n".join(body).encode()).hexdigest()
            name = None
        elif name:
            line = NUMBERED.sub(lambda k: ".L" + k.group(1), line.split(";")[0]).strip()
            if line:
                body.append(line)


def digest(src):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "a.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", asm, src],
                       check=True, capture_output=True)
        with open(asm) as f:
            return ["%s %s %s" % (os.path.basename(src), n, h) for n, h in functions(f.read())]


def main(argv):
    summary = "--summary" in argv
    if summary:
        argv.remove("--summary")
    jobs = int(argv.pop(argv.index("-j") + 1)) if "-j" in argv else 4
    if "-j" in argv:
        argv.remove("-j")
    csrc = argv[0] if argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kws_amd", "csrc")
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        lines = [l for ls in ex.map(digest, sorted(glob.glob(os.path.join(csrc, "*.hip")))) for l in ls]
    lines.sort()
    if summary:
        by_source = {}
        for l in lines:
            by_source.setdefault(l.split()[0], []).append(l)
        lines = ["%s %d %s" % (src, len(ls), hashlib.sha256("\n".join(ls).encode()).hexdigest())
                 for src, ls in sorted(by_source.items())]
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Compare the instruction streams of every step-kernel instantiation (hlx_env_kernel<...>) of two builds of libhlx.so,
without a GPU: `python tools/isa_step_diff.py [--all] OLD.so NEW.so`.  `--all`: every kernel of the code objects (observation,
evaluation, HRL and self-test kernels as well).  Addresses and the scratch file names of the code objects are ignored; exit
status 1 if a kernel is missing or differs.  For changes that must leave the step kernel (or, with --all, every kernel) alone."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hlynr_intercept_amd import hotcheck  # noqa: E402


def kernels(path, every=False):
    out, cur = {}, None
    for line in hotcheck.listing(path).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1) if every or "hlx_env_kernel" in m.group(1) else None
            if cur:
                out[cur] = []
        elif cur and "file format" not in line:
            out[cur].append(re.sub(r"^\s*[0-9a-f]+:\s*", "", line))
    return out


def main(argv):
    every = "--all" in argv
    old, new = [a for a in argv if a != "--all"][:2]
    a, b = kernels(old, every), kernels(new, every)
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("DIFFERS" if k in a and k in b else "ONLY IN " + ("OLD" if k in a else "NEW"), k)
    what = "kernels" if every else "step-kernel instantiations"
    print(f"{len(set(a) & set(b)) - len([k for k in bad if k in a and k in b])} of {len(set(a) | set(b))} {what} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

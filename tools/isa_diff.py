#!/usr/bin/env python3
"""isa_diff.py OLD.s NEW.s - did a source change touch the generated gfx950 code?

Both files are assembly of csrc/dib_api.hip as tests/_isa.py compiles it (hipcc --offload-arch=gfx950 -O3 -std=c++17 -S
--cuda-device-only).  Prints every kernel that only one file has and every kernel whose code differs (tests/_isa.py
fingerprint: comments and the numbering of local labels do not count), with the resource statistics of tests/_isa.py parse
before and after.  Prints nothing and exits 0 when the device code is the same - what a refactor of host code must show -
and exits 1 otherwise."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _isa  # noqa: E402


def main(old_path, new_path):
    texts = [open(p).read() for p in (old_path, new_path)]
    (old_fp, new_fp), (old_st, new_st) = map(_isa.fingerprint, texts), map(_isa.parse, texts)
    changed = 0
    for name in sorted(set(old_fp) | set(new_fp)):
        if old_fp.get(name) == new_fp.get(name):
            continue
        changed += 1
        a, b = old_st.get(name), new_st.get(name)
        print("%s %s" % ("only in OLD:" if name not in new_fp else "only in NEW:" if name not in old_fp else "differs:", name))
        for key in sorted(set(a or ()) | set(b or ())):
            va, vb = (a or {}).get(key), (b or {}).get(key)
            print(("    %-14s %8s -> %-8s%s" % (key, "-" if a is None else va, "-" if b is None else vb, "" if va == vb else "   <--")).rstrip())
    if changed:
        print("%d of %d kernels differ" % (changed, len(set(old_fp) | set(new_fp))))
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

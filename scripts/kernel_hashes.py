"""SHA-256 of every kernel's machine code in the library (or two libraries
compared).

usage: python scripts/kernel_hashes.py [LIB]            -> JSON {symbol: sha256}
       python scripts/kernel_hashes.py OLD.json LIB     -> per-kernel same / DIFFERENT

Used to show that a source change (e.g. retiring A/B macros from the kernel
sources) left every shipped kernel's code as it was."""
import json
import os
import sys
import hashlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from syncfast_amd._lib import LIB_PATH, _code_objects, _kernel_symbols  # noqa: E402


def hashes(path):
    return {nm: hashlib.sha256(code).hexdigest()
            for _, co in _code_objects(path) for nm, st_info, code in _kernel_symbols(co)
            if (st_info & 0xF) == 2 and not nm.endswith(".kd")}  # STT_FUNC


def main():
    if len(sys.argv) == 3:
        old = json.load(open(sys.argv[1]))
        new = hashes(sys.argv[2])
        ok = True
        for k in sorted(set(old) | set(new)):
            st = "same" if old.get(k) == new.get(k) else ("REMOVED" if k not in new else
                                                        "ADDED" if k not in old else "DIFFERENT")
            ok &= st == "same"
            print(f"{st:9s} {k}")
        sys.exit(0 if ok else 1)
    print(json.dumps(hashes(sys.argv[1] if len(sys.argv) > 1 else LIB_PATH), indent=1, sort_keys=True))


if __name__ == "__main__":
    main()

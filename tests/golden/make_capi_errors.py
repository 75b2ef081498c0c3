"""Record tests/golden/capi_errors.json: the (status, last_error) of every case of
tests/capi_errors_cases.py on a host handle of the library given.

    python tests/golden/make_capi_errors.py PATH/TO/libtgms.so

The fixture pins what the entry points answer to bad arguments, so it is recorded from the build
of the commit BEFORE a change to the C-ABI layer (a worktree of the parent commit, built there),
never from the tree under test; tests/test_capi_errors_host.py then holds the tree to it, status
and message, byte for byte.  No GPU is needed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from trajectory_generator_ros2_amd import _lib  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    L = _lib.load(os.path.abspath(sys.argv[1]))  # the first load decides the library of the process
    import capi_errors_cases as CE
    got = CE.run_all(L)
    packed = CE.pack(got)
    assert CE.unpack(packed) == got
    with open(os.path.join(HERE, "capi_errors.json"), "w") as f:  # one line per entry point
        f.write('{"messages": %s,\n "cases": {\n' % json.dumps(packed["messages"]))
        f.write(",\n".join("  %s: %s" % (json.dumps(e), json.dumps(c, separators=(",", ":")))
                           for e, c in sorted(packed["cases"].items())))
        f.write("}}\n")
    print(len(got), "cases")


if __name__ == "__main__":
    main()

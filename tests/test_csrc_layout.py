"""The layout of csrc/ ("File map of csrc/"), as a text scan of the sources: every kernel is
compiled by a launch unit, the host (the Makefile's HOST list, compiled as plain C++) holds no device code,
and the Makefile's lists name the files that exist.  No compiler is run."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed_sudoku_solver_amd",
                    "csrc")


def read(path):
    with open(path) as f:
        return f.read()


def names(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, pattern)))


def code(text):
    """the text without // comments (a comment may speak of kernels)"""
    return re.sub(r"//[^\n]*", "", text)


def includes(text):
    return set(re.findall(r'#include\s+"([^"]+)"', text))


def make_list(var):
    """the words of a Makefile variable assigned with :=, continuation lines joined"""
    m = re.search(r"^%s\s*:=\s*((?:[^\n]*\\\n)*[^\n]*)" % var, read(os.path.join(CSRC, "Makefile")), re.M)
    assert m, var
    return m.group(1).replace("\\\n", " ").split()


def test_every_kernel_header_is_compiled_by_a_launch_unit():
    units = names("*_launch.hip")
    assert units
    for h in names("*_kernel.h"):
        if "__global__" not in code(read(os.path.join(CSRC, h))):
            continue
        direct = [u for u in units if h in includes(read(os.path.join(CSRC, u)))]
        assert direct, "%s defines a kernel and no *_launch.hip includes it" % h
    # and nothing but the launch units (and the kernel headers) defines one
    for f in names("*.hip") + names("*.h") + names("*.cpp"):
        if not f.endswith(("_launch.hip", "_kernel.h")):
            assert "__global__" not in code(read(os.path.join(CSRC, f))), f


def test_host_sources_hold_no_device_code():
    host = [h + ".hip" for h in make_list("HOST")]
    assert host
    for f in host + ["launch.h"] + names("*_args.h"):
        text = code(read(os.path.join(CSRC, f)))
        assert "__global__" not in text and "<<<" not in text and "threadIdx" not in text, f
        assert not [h for h in includes(text) if h.endswith("_kernel.h")], f


def test_makefile_lists_name_the_files():
    units, host = make_list("UNITS"), make_list("HOST")
    assert len(set(units)) == len(units) and len(set(host)) == len(host)
    assert sorted(u + ".hip" for u in units) == names("*_launch.hip")
    assert sorted(f + ".hip" for f in units + host) == names("*.hip")

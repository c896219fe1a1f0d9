"""Every BOD_* environment switch the library reads must have a user outside csrc/: a test or tool under tests/, bench.py, a package
Python file or a public document.  A switch nobody names selects a code path that is neither measured nor exercised -- a finished
experiment left behind as an option."""
import os
import re

from conftest import ROOT

PKG = os.path.join(ROOT, "bayes-od-rc_amd")
GETENV = re.compile(r'getenv\("(BOD_[A-Z0-9_]+)"')
BINARY = (".npz", ".npy", ".pyc", ".so", ".o")


def _files(top, keep=lambda name: True):
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for n in names:
            if keep(n) and not n.endswith(BINARY):
                yield os.path.join(d, n)


def _read(path):
    with open(path, errors="ignore") as fp:
        return fp.read()


def test_every_switch_has_a_user_outside_csrc():
    switches = set()
    for path in _files(os.path.join(PKG, "csrc")):
        switches.update(GETENV.findall(_read(path)))
    assert len(switches) >= 10, "no getenv(\"BOD_...\") found under csrc/: the pattern no longer matches the sources"
    users = list(_files(os.path.join(ROOT, "tests")))
    users += [p for p in _files(PKG, lambda n: n.endswith(".py")) if os.sep + "csrc" + os.sep not in p]
    users += [os.path.join(ROOT, f) for f in ("bench.py", "README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "bayesod.h"))]
    text = "\n".join(_read(p) for p in users)
    named = set(re.findall(r"BOD_[A-Z0-9_]+", text))          # whole names: BOD_X does not count as a use of BOD_X_Y or the reverse
    unused = sorted(switches - named)
    assert not unused, "switches read in csrc/ that no test, tool, benchmark, package file or public document names: %s" % ", ".join(unused)

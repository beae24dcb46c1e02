"""kimimaro_amd.build without a GPU or a compiler: every file the library is compiled from is a file needs_build() watches, so a
header that somebody adds under csrc/ cannot silently stop triggering rebuilds."""
import glob
import os
import re

from kimimaro_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.MULTILINE)


def test_every_quoted_include_is_watched():
    watched = {os.path.realpath(os.path.join(build.CSRC, d)) for d in build.DEPS}
    files = sorted(glob.glob(os.path.join(build.CSRC, "*.hip")) + glob.glob(os.path.join(build.CSRC, "*.h")))
    assert {os.path.basename(f) for f in files} >= set(build.SOURCES)
    seen = 0
    for f in files:
        assert os.path.realpath(f) in watched, "%s is compiled but not watched" % os.path.basename(f)
        for name in INCLUDE.findall(open(f).read()):
            target = os.path.realpath(os.path.join(os.path.dirname(f), name))
            assert os.path.isfile(target), "%s includes %s, which does not exist" % (os.path.basename(f), name)
            assert target in watched, "%s includes %s, which needs_build() does not watch" % (os.path.basename(f), name)
            seen += 1
    assert seen >= len(build.SOURCES)        # (every source includes common.h at least: the pattern still finds includes)

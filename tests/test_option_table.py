"""The option table of hdb_ctx_set_option (csrc/options.cpp), the defaults the tests restore
(path_helpers.DEFAULTS) and DESIGN.md's table of where each option is pinned name the same
options: a new option without a test row, or a removed one still listed, fails here."""
import os
import re

from conftest import PKG_NAME, ROOT
from path_helpers import DEFAULTS


def accepted_options():
    with open(os.path.join(ROOT, PKG_NAME, "csrc", "options.cpp")) as fh:
        src = fh.read()
    table = src[src.index("const Option OPTIONS[] = {"):src.index("}  // namespace")]
    return set(re.findall(r'^    \{"([a-z0-9_]+)", ', table, re.M))


def test_defaults_cover_the_option_table():
    assert accepted_options() == set(DEFAULTS)


def test_design_lists_every_option():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        doc = fh.read()
    table = doc[doc.index("**Runtime options and where each is pinned.**"):doc.index("## 5. Measurement")]
    listed = set(re.findall(r"`([a-z0-9_]+)`", table))
    assert accepted_options() <= listed, sorted(accepted_options() - listed)

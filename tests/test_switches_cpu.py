"""The environment switches the package reads are the ones INTEGRATION.md lists ("Environment switches", first table)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video_distillation_amd")
READ = re.compile(r'(?:environ\.get\(|environ\[|getenv\()\s*"(VD_[A-Z0-9_]+)"')


def test_integration_md_lists_exactly_the_switches_the_package_reads():
    paths = glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True) + \
        [p for p in glob.glob(os.path.join(PKG, "csrc", "*")) if os.path.isfile(p)]
    read = set()
    for path in paths:
        with open(path, encoding="utf-8", errors="replace") as f:
            read.update(READ.findall(f.read()))
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        section = f.read().split("### Environment switches", 1)[1]
    table = section[section.index("| name |"):].split("\n\n", 1)[0]          # the first table ends at the first blank line
    listed = set(re.findall(r"^\| `(VD_[A-Z0-9_]+)` \|", table, flags=re.M))
    assert len(read) > 20, "the search found no reads: has the package moved?"
    assert read == listed, "read but not listed: %s; listed but not read: %s" % (sorted(read - listed), sorted(listed - read))

"""The SLAMHIP_* runtime options, checked on the sources (no GPU, no build): every option is read through the helpers of
common.h, each at exactly one place, and INTEGRATION.md's switch table lists exactly the options the sources read."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam.net_amd", "csrc")
HELPER_CALL = re.compile(r'\bsh_env_(?:set|int|real|str)\(\s*"(SLAMHIP_[A-Z0-9_]+)"')


def _sources():
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            yield name, f.read()


def _helper_reads():
    reads = []
    for name, text in _sources():
        for lineno, line in enumerate(text.splitlines(), 1):
            reads += [(m.group(1), "%s:%d" % (name, lineno)) for m in HELPER_CALL.finditer(line)]
    return reads


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    section = re.search(r"^## 7\. Runtime switches.*?(?=^## |\Z)", text, re.M | re.S)
    assert section, "INTEGRATION.md has no runtime switch section"
    names = set()
    for line in section.group(0).splitlines():
        if line.startswith("| `"):
            names |= set(re.findall(r"`(SLAMHIP_[A-Z0-9_]+)", line.split("|")[1]))
    return names


def test_getenv_only_in_helpers():
    stray = []
    for name, text in _sources():
        for lineno, line in enumerate(text.splitlines(), 1):
            if "getenv(" in line and not (name == "common.h" and line.startswith("static inline") and "sh_env_" in line):
                stray.append("%s:%d: %s" % (name, lineno, line.strip()))
    assert not stray, "\n".join(stray)


def test_each_option_read_once():
    sites = {}
    for opt, where in _helper_reads():
        sites.setdefault(opt, []).append(where)
    assert sites, "no option reads found"
    multi = {opt: w for opt, w in sites.items() if len(w) > 1}
    assert not multi, multi


def test_switch_table_matches_sources():
    read = {opt for opt, _ in _helper_reads()}
    documented = _documented()
    assert read - documented == set(), "read but not in INTEGRATION.md: %s" % sorted(read - documented)
    assert documented - read == set(), "in INTEGRATION.md but never read: %s" % sorted(documented - read)

"""The "Environment settings" table of INTEGRATION.md lists exactly the B2P_* variables the package, csrc/
and run.py read: a switch added without a row, or a row whose switch is gone, fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the name inside an environment read; tied to the call, so macros (B2P_CHECK_ARG, B2P_EPI_C16_FP16) and
# names in comments do not match
_READ = re.compile(r'(?:os\.environ\.get\(|os\.environ\[|getenv\()\s*"(B2P_[A-Z0-9_]+)"')


def _read_in_code() -> set:
    pkg = os.path.join(ROOT, "wav2vec2forbrain_amd")
    files = glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)
    files += [f for f in glob.glob(os.path.join(pkg, "csrc", "*")) if os.path.isfile(f)]
    files.append(os.path.join(ROOT, "run.py"))
    names = set()
    for path in files:
        with open(path, encoding="utf-8") as f:
            names.update(_READ.findall(f.read()))
    return names


def _documented() -> set:
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    section = text.split("## Environment settings", 1)[1].split("\n## ", 1)[0]
    return set(re.findall(r"^\| `(B2P_[A-Z0-9_]+)` \|", section, re.M))


def test_env_table_matches_code():
    code, doc = _read_in_code(), _documented()
    assert code, "no environment reads found: the pattern no longer matches the code"
    assert code - doc == set(), f"read in code, missing from INTEGRATION.md: {sorted(code - doc)}"
    assert doc - code == set(), f"in INTEGRATION.md, read nowhere: {sorted(doc - code)}"

"""Every scratch slot has one owning source file (qampy_amd/csrc/common.h `enum class Slot`): two units that shared a slot would overwrite one
another's buffers as soon as they ran on different streams of one host thread.  Static check of the sources; no GPU, no build."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qampy_amd", "csrc")

# the lookahead and the block-iterative trainer are two forms of one trainer in one translation unit; a call runs one of them
SHARED = {"GRAM": {"train_bi.h", "train_la.h"}}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _enumerators():
    text = open(os.path.join(CSRC, "common.h")).read()
    body = re.search(r"enum\s+class\s+Slot\s*:\s*int\s*\{(.*?)\};", text, flags=re.S).group(1)
    names = re.findall(r"\b([A-Z][A-Z0-9_]*)\b\s*(?:=\s*[^,]+)?(?:,|$)", _strip_comments(body).strip())
    assert names and names[-1] == "COUNT", names
    assert len(set(names)) == len(names), names
    return names[:-1]


def _sources():
    files = [f for pat in ("*.hip", "*.h", "*.inc") for f in glob.glob(os.path.join(CSRC, pat))]
    return {os.path.basename(f): _strip_comments(open(f).read()) for f in files if os.path.basename(f) != "common.h"}


def test_every_slot_has_one_owner():
    slots = _enumerators()
    assert len(slots) >= 30
    src = _sources()
    for name in slots:
        users = {f for f, text in src.items() if re.search(r"\bSlot::%s\b" % name, text)}
        if name in SHARED:
            assert users == SHARED[name], "Slot::%s is used in %s" % (name, sorted(users))
        else:
            assert len(users) == 1, "Slot::%s is used in %s" % (name, sorted(users))
    # nothing names a slot that the enum does not have
    named = {m for text in src.values() for m in re.findall(r"\bSlot::([A-Za-z0-9_]+)", text)}
    assert named <= set(slots) | {"COUNT"}, sorted(named - set(slots))


def test_no_numeric_slot_argument():
    for f, text in _sources().items():
        assert not re.search(r"\bscratch\s*\(\s*(?:\(\s*Slot\s*\)\s*)?[0-9]", text), f
        assert "static_cast<Slot>" not in text and "(Slot)" not in text, f

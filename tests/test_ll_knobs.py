"""LunarLander's environment knobs are one table (kLLKnobs, lunar_lander.hip): the names the suite and tools/ use, the rows of that
table and the knobs= line of mgym_get_info must be the same set, and nothing else in that file may read the environment."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = re.compile(r"MGYM_LL_[A-Z0-9_]+")
TEXT = (".py", ".sh", ".md", ".hip", ".c", ".h")


def source():
    return open(os.path.join(ROOT, "modurl_gym_amd", "csrc", "lunar_lander.hip"), encoding="utf-8").read()


def names_used_by_tests_and_tools():
    used = set()
    for top in ("tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(TEXT):
                    used |= set(KNOB.findall(open(os.path.join(d, f), encoding="utf-8", errors="replace").read()))
    return used


def test_knob_table_info_line_and_users_agree():
    src = source()
    table = re.search(r"kLLKnobs\[\] = \{\n(.*?)\n\};", src, re.S).group(1)
    rows = re.findall(r'^\s*\{"(MGYM_LL_[A-Z0-9_]+)", &LLOptions::', table, re.M)
    assert len(rows) == len(table.splitlines()) == len(set(rows)), "one row per knob, one knob per row"
    # mgym_get_info: the knobs= line is written from the table and from nothing else ...
    assert src.count("knobs=\"") == 1
    assert re.search(r'"\\nknobs=";\n\s*for \(const LLKnob& k : kLLKnobs\) out \+= [^;\n]*k\.name;', src)
    # ... so no knob name stands in a string of its own anywhere outside the table
    assert sorted(re.findall(r'"(MGYM_LL_[A-Z0-9_]+)"', src)) == sorted(rows)
    assert set(rows) == names_used_by_tests_and_tools()


def test_the_environment_is_read_in_one_place():
    src = source()
    reader = re.search(r"static LLOptions ll_read_options\(\) \{\n(.*?)\n\}\n", src, re.S).group(1)
    assert src.count("getenv") == reader.count("getenv") == 1

"""CPU: every `T2V_*` variable the package reads from the environment has a row in the switch table of INTEGRATION.md, and the
table lists nothing that is no longer read — a new switch, or one left behind by its code, shows up here. Reads files only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r'(T2V_[A-Z0-9_]+)'
PY_READS = (re.compile(r'os\.environ\.get\(\s*[\'"]' + NAME), re.compile(r'os\.environ\[\s*[\'"]' + NAME))
HIP_READS = (re.compile(r'\b(?:getenv|env_long)\(\s*"' + NAME),)


def _read_in_code():
    pkg = os.path.join(ROOT, 'txt2vid_amd')
    names = set()
    for paths, patterns in ((glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True), PY_READS),
                            (glob.glob(os.path.join(pkg, 'csrc', '*.hip')), HIP_READS)):
        assert paths
        for path in paths:
            with open(path) as f:
                text = f.read()
            for pat in patterns:
                names.update(pat.findall(text))
    return names


def _listed_in_table():
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        lines = f.read().splitlines()
    start, = [i for i, l in enumerate(lines) if l.startswith('## Environment switches')]
    names, rows = set(), 0
    for l in lines[start + 1:]:
        if l.startswith('## '):
            break
        if l.startswith('|') and not l.startswith('|---') and not l.startswith('| variable'):
            names.update(re.findall(NAME, l.split('|')[1]))
            rows += 1
    assert rows
    return names


def test_switch_table_lists_exactly_the_variables_the_package_reads():
    read, listed = _read_in_code(), _listed_in_table()
    assert read == listed, 'read under txt2vid_amd/ but missing from the switch table of INTEGRATION.md: %s; listed there but read nowhere: %s' \
        % (sorted(read - listed), sorted(listed - read))

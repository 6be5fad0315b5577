"""The command lines of `hifimeth-hip pileup` and `hifimeth-hip diff`, replayed from tests/golden/cli_options.json (recorded by
tools/make_cli_options.py): exit code, the text before the usage, the usage text and the `Parameters:` echo, byte for byte.  Every
case names files that do not exist and ends before an engine is created, so none needs a GPU."""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_cli_options as M  # noqa: E402

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


@pytest.fixture(scope="module")
def fixture():
    return M.load()


def test_every_case_of_the_fixture(fixture, tmp_path):
    usage, cases = fixture
    prefix = str(tmp_path / "out")
    for cmd, text in usage.items():
        assert M.run_case(CLI, cmd, ["-h"], prefix) == (0, text, "")
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(lambda c: M.run_case(CLI, c[0], c[1], prefix), cases))
    wrong = []
    for (cmd, args, code, follows, stderr), have in zip(cases, got):
        want = (code, usage[cmd] if follows else None, stderr)
        if have != want:
            wrong.append((cmd, args, want[0], want[2], have[0], have[2], "usage differs" if have[1] != want[1] else ""))
    assert not wrong, (len(wrong), wrong[:5])
    assert not os.listdir(tmp_path)        # no case creates a file


def test_fixture_is_the_generators_matrix_and_names_every_flag(fixture):
    """The fixture holds exactly the generator's matrix, and per flag that the usage text of a command lists the matrix has a case
    that ends in the usage text and one that gets past the checks: a new option needs its cases.  The flags come from the fixture's
    usage text, which is the binary's own: test_every_case_of_the_fixture compares the two."""
    usage, cases = fixture
    assert [(c[0], c[1]) for c in cases] == sorted(M.matrix(), key=lambda c: c[0] != "pileup")
    for cmd, text in usage.items():
        flags = re.findall(r"^  (-\w)(?: |$)", text, re.M)
        assert len(flags) == len(set(flags)) >= 8, flags
        for flag in flags:
            ends = {c[3] for c in cases if c[0] == cmd and flag in c[1]}
            assert ends == {0, 1}, (cmd, flag)

#!/usr/bin/env python3
"""Record what `hifimeth-hip pileup` and `hifimeth-hip diff` do with their command lines: tests/golden/cli_options.json; and what
`hifimeth-hip smooth` does with its: tests/golden/cli_options_smooth.json, a file of the same form.

Every case names input files that do not exist, so a bad command line ends in the usage text, a good `pileup` one at
`ERROR: cannot open no.bam` after the whole `Parameters:` echo, and a good `diff` or `smooth` one after its echo at "no context has a
cov.bed file of both samples" (`smooth`: "of the sample").  No case writes a file or creates an engine, so the matrix runs without a GPU in a few seconds.

Per command the fixture holds rows [arguments after the command word, exit code, 1 if the usage text follows, stderr before `USAGE:`
(all of it when there is none)].  What repeats is stored once: the `-h` text of each command; the frame of its echo without options
(the lines down to `output prefix:` and what follows them stand in a row as <HEAD> and <TAIL>); and the texts in front of the usage,
which a row names by their index in "messages".  The executable's path, its directory and the output prefix are replaced by the
tokens EXE, EXEDIR and PREFIX.  tests/test_cli_options_cpu.py replays the file (load() undoes the folding).
tests/test_pileup_smooth_cpu.py replays the second file.  matrix() and record() take the commands of the first file unless told
otherwise; the first file comes out of this tool byte for byte as it was before `smooth` had its own.

usage: python tools/make_cli_options.py [path of hifimeth-hip]      (default: hifimeth_amd/bin/hifimeth-hip of this tree)
"""
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_options.json")
POSITIONALS = {"pileup": ["ref.fa", "no.bam", "PREFIX"], "diff": ["ref.fa", "a", "b", "PREFIX"], "smooth": ["ref.fa", "a", "PREFIX"]}
SMOOTH_FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_options_smooth.json")
COMMANDS = ("pileup", "diff")          # the commands of FIXTURE
SMOOTH_COMMANDS = ("smooth",)          # ... and of SMOOTH_FIXTURE

LLMAX = 9223372036854775807
JUNK = ["x", "5x", "2.5", "", " 5", "+5", "-3", str(LLMAX + 1)]   # the last one: ERANGE
FLOATS = ["nan", "inf", "1e-2"]


def ends(lo, hi):
    """both ends of an integer range and one step outside each"""
    return [str(v) for v in (lo - 1, lo, hi, hi + 1)]


# flag -> (the options that make it legal, its values beyond JUNK); a flag that takes no value has None
LENIENT = ("-q", "-f", "-t", "-d", "-b", "-l", "-p", "-T", "-m", "-B", "-R")   # atoi, atof or any text: JUNK has nothing to show
PILEUP = {
    "-H": ([], None), "-A": (["-H"], None), "-Q": (["-H", "-A"], None), "-G": (["-H", "-A"], None), "-D": ([], None), "-M": ([], None),
    "-K": ([], None),
    "-q": ([], ["0", "20", "-1"]), "-f": ([], ["0", "0.85", "85"] + FLOATS), "-t": ([], ["0", "1", "16"]), "-d": ([], ["0", "3", "-1"]),
    "-b": ([], ["0", "1", "4096"]),
    "-a": (["-H", "-A"], ends(1, 2147483647)),
    "-s": (["-H", "-A", "-G"], ["0", "1e-300", "1e-400", "0.05", ".1", "1", "1.0000001", "1.", "0x1p-4"] + FLOATS),
    "-g": (["-H", "-A", "-G"], ends(1, LLMAX)), "-n": (["-H", "-A", "-G"], ends(1, 2147483647)),
    "-B": ([], ["chrC"]),
    "-e": ([], ["0,0,0", "1,1,1", "0.01,nan,0.5", "nan,nan,nan", ".5,.5,.5", "1e-2,0,0", "1.1,0,0", "-0.1,0,0", "0,0", "0,0,0,0", "inf,0,0",
                ",0,0", "+1,0,0", "0,0,", "0, 0,0", "0,0,1e400"]),
    "-u": (["-D"], ["0.2:0.7", "0.2:0.7,0.1:0.5,0.05:0.3", "nan,0.1:0.5,nan", "1e-1:8e-1", "0.5:0.5", "0.5:0.50000000001", "0.7:0.2", "0:0.5",
                    "0.2:1", "0.2", "0.2:0.7,0.1:0.5", "0.2:0.7,0.1:0.5,0.05:0.3,0.1:0.2", ":", "0.2:", ":0.7", "0.2:0.7:0.9", "0.2:0.7,", "+0.2:0.7",
                    "-0.2:0.7"] + FLOATS),
    "-x": (["-D"], ["-0.5", "-0", "0", "12.5", "256", "256.5", "1e400"] + FLOATS), "-j": (["-D"], ends(1, LLMAX)),
    "-Y": (["-D"], ends(1, LLMAX)),
    "-E": ([], ends(2, 4)), "-w": (["-E", "3"], ends(1, 65536)), "-o": (["-E", "3"], ends(1, LLMAX)),
    "-v": (["-M"], ends(0, LLMAX)),
    "-L": ([], ends(2, 16384)), "-z": (["-L", "100"], ends(0, LLMAX)),
    "-P": ([], ends(1, 2048)), "-y": (["-P", "10"], ends(0, LLMAX)),
    "-I": ([], ["0", "5", "5:7", "0:0", "0:9", "2147483647", "2147483648", "5:2147483647", "5:2147483648", "5:", ":5", "5:7:9", "5:x", "5:-1", "5: 7"]),
    "-R": ([], ["iv.bed"]), "-C": (["-R", "iv.bed"], ends(1, LLMAX)),
    "-J": (["-R", "iv.bed"], ["0", "1", "10", "1000", "1001", "10:100:10", "10:100:3", "10:0:0", "10:100:0", "10:0:5", "10:100", "10:1000:1000",
                              "10:1001:1001", "10:100:10:1", "10:", "10:x:1", "10:100:-10"]),
    "-S": ([], ends(0, 3)), "-O": (["-S", "1"], ends(1, LLMAX)),
    "-m": (["-K"], ["models"]), "-c": (["-K"], ["cpg", "chg,chh", "cpg,chg,chh", "CpG", "all", "xyz", "cpg,", ",", "cpg,cpg"]),
    "-l": (["-K"], ["-1", "0", "500"]), "-p": (["-K"], ends(0, 2)), "-T": (["-K"], ["-2", "-1", "0", "1", "2"]),
}
DIFF = {
    "-Q": ([], None), "-G": ([], None),
    "-a": ([], ends(1, 2147483647)), "-s": (["-G"], PILEUP["-s"][1]), "-g": (["-G"], ends(1, LLMAX)), "-n": (["-G"], ends(1, 2147483647)),
    "-t": ([], ["0", "1", "16"]), "-d": ([], ["0", "3", "-1"]),
}

# hand-written command lines: options without their parent, each group's precedence, two groups bad at once, argument shape
PILEUP_LINES = [
    # without the parent, with a good value and with a bad one
    "-A", "-Q", "-G", "-H -Q", "-H -G", "-a 5", "-a 0", "-A -a 5", "-Q -a 5", "-Q -G", "-H -A -Q -a 0", "-G -s .1", "-s .1", "-g 5", "-n 5",
    "-s 2", "-H -A -s 2", "-H -A -n x", "-H -A -G -a 0 -s 2", "-A -s x", "-H -A -G -s 2 -g 5", "-H -A -G -g 5 -s 2",
    "-m d", "-c cpg", "-c xyz", "-l 5", "-l -1", "-p 1", "-p 3", "-T 1", "-T 2", "-K -l -1 -p 3", "-K -p 3 -T 2", "-K -p 3 -l -1",
    "-w x -z -1", "-z -1 -w x", "-B c -e 0,0,0", "-e 0,0,0 -B c", "-B c -e x", "-e x -B c", "-e x -w x", "-w x -e x",
    "-u .1:.8", "-u x", "-x 5", "-x 300", "-j 5", "-j 0", "-Y 5", "-Y 0", "-Y x", "-u x -Y 0", "-Y 0 -u x", "-D -Y 0 -u x", "-D -u x -Y 0",
    "-D -u 0.5:0.5 -Y 0", "-D -x 300 -u nan",
    "-w 5", "-w x", "-o 5", "-o 0", "-E 5 -w 5", "-E x -w 5", "-E 3 -E x", "-E x -E 3", "-E 2 -E 4",
    "-v 1", "-v -1", "-v x", "-M -v 1 -v x", "-M -v x -v 1",
    "-z 1", "-z -1", ["-z", "-1 "], ["-L", "100", "-z", " 1"], "-z x", "-L 1 -z 1", "-L 5 -L 100",
    "-y 1", "-y -1", "-y x", "-I x", "-I 5 -y 1", "-I x -y 1", "-P 10 -I x",
    "-C 2", "-C 0", "-C x", "-J 10", "-J 0", "-J 10 -C 2", "-R iv.bed -C 2 -J 0", "-R iv.bed -R other.bed",
    "-O 2", "-O 0", "-O x", "-S 4 -O 2", "-S 1 -S 4",
    # argument shape
    "!", "!-h", "!-H -h", "!-w x -h", "!-h -w x", "!-e x -h", "!-h -e x", "!-c xyz -h", "!-Z 1 -h", "-n -h", "!-H -A -G -n ref.fa no.bam PREFIX",
    "!-n", "!-H", "!-H -n", "!ref.fa no.bam PREFIX -n", "-Z 1", "!-Z", "-Z", "-ab 5", "--help 1", "!--help", "-HA 1", "-H5 1",
    "!- ref.fa no.bam PREFIX", "!a ref.fa no.bam PREFIX", "!-H a ref.fa no.bam PREFIX", "!ref.fa -H no.bam PREFIX", "!ref.fa no.bam PREFIX -H",
    "!ref.fa", "!ref.fa no.bam", "!ref.fa no.bam PREFIX more", "!-H ref.fa no.bam", "!-w x ref.fa no.bam", "!-Z 1 ref.fa no.bam",
    # good lines: each output that echoes, then all of them with values that are not the defaults
    "", "-q 20 -f 0.85 -t 3 -d 1 -b 64", "-H", "-H -A", "-H -A -a 7", "-H -A -Q", "-H -A -G", "-H -A -G -s 0.05 -g 250 -n 4", "-B chrC",
    "-e 0.01,nan,0.5", "-D", "-D -u 0.2:0.7 -x 12.5 -j 2000", "-D -u nan,0.1:0.5,nan", "-D -Y 7", "-E 3", "-E 4 -w 200 -o 5", "-M", "-M -v 0",
    "-H -M", "-L 100", "-L 100 -z 0", "-P 10", "-P 10 -y 0", "-I 5", "-I 5:7", "-I 0:7", "-R iv.bed", "-R iv.bed -C 3", "-R iv.bed -J 10",
    "-R iv.bed -J 10:100:5", "-S 0", "-S 2 -O 4", "-K", "-K -m models -c cpg,chh -l 500 -p 2 -T 0", "-K -T 1", "-K -T -1", "-K -c chg",
    "-q 20 -f 0.85 -t 3 -d 1 -b 64 -H -A -a 7 -Q -G -s 0.05 -g 250 -n 4 -B chrC -D -u 0.2:0.7,0.1:0.5,nan -x 12.5 -j 2000 -Y 7 -E 4 -w 200 "
    "-o 5 -M -v 0 -L 100 -z 0 -P 10 -y 0 -I 5:7 -R iv.bed -C 3 -J 10:100:5 -S 2 -O 4 -K -m models -c cpg,chh -l 500 -p 2 -T 0",
]
DIFF_LINES = [
    "-s .1", "-g 5", "-n 5", "-s 2", "-s x", "-n x", "-a 0 -s .1", "-s .1 -a 0", "-G -a 0 -s 2", "-G -s 2 -g 5", "-G -g 5 -s 2",
    "!", "!-h", "!-Q -h", "!-s x -h", "!-h -s x", "!-Z 1 -h", "-n -h", "!-G -n ref.fa a b PREFIX", "!-n", "!-Q", "!-G -n", "-Z 1", "!-Z", "-Z",
    "-ab 5", "--help 1", "-H 1", "-A 1", "-q 5", "-K 1", "-QG 1", "!- ref.fa a b PREFIX", "!a ref.fa a b PREFIX b", "!ref.fa -Q a b PREFIX",
    "!ref.fa", "!ref.fa a b", "!ref.fa a b PREFIX more", "!-Q ref.fa a b", "!-s x ref.fa a b", "!-Z 1 ref.fa a b",
    "", "-Q", "-G", "-a 7", "-t 3 -d 1", "-G -s 0.05 -g 250 -n 4", "-t 3 -d 1 -a 7 -Q -G -s 0.05 -g 250 -n 4",
]
SMOOTH = {
    "-W": ([], ends(1, 16384) + ["500"]), "-a": ([], ends(1, 2147483647)), "-i": ([], ends(1, LLMAX)),
    "-t": ([], ["0", "1", "16"]), "-d": ([], ["0", "3", "-1"]),
}
SMOOTH_LINES = [
    "-W x -a 0", "-a 0 -W x", "-i 0 -t 3", "-W 16 -W 0", "-W 0 -W 16",
    "!", "!-h", "!-W 7 -h", "!-W x -h", "!-h -W x", "!-Z 1 -h", "-i -h", "!-W", "!-W 7 -i", "-Z 1", "!-Z", "-Z", "-Wa 5", "--help 1", "-H 1", "-Q 1",
    "-s .1", "-q 5", "!- ref.fa a PREFIX", "!a ref.fa a PREFIX b", "!ref.fa -W a PREFIX", "!ref.fa", "!ref.fa a", "!ref.fa a PREFIX more",
    "!-W 7 ref.fa a", "!-W x ref.fa a", "!-Z 1 ref.fa a",
    "", "-W 16", "-W 16384 -a 3 -i 5", "-t 3 -d 1", "-t 3 -d 1 -W 1 -a 2 -i 2",
]
# one way to make each pileup check fire, in the order the checks run: neighbours go into the matrix in both orders
GROUP_BAD = ["-A", "-l 5", "-B c -e 0,0,0", "-u .1:.8", "-w x", "-v 1", "-z -1", "-y x", "-C 2", "-O 0"]


def matrix(commands=COMMANDS):
    """[(command, [arguments])] of `commands`, without duplicates, in a fixed order"""
    cases = []

    def add(cmd, args, positionals=True):
        case = (cmd, list(args) + (POSITIONALS[cmd] if positionals else []))
        if case not in cases:
            cases.append(case)

    for cmd, table, lines in (("pileup", PILEUP, PILEUP_LINES), ("diff", DIFF, DIFF_LINES), ("smooth", SMOOTH, SMOOTH_LINES)):
        if cmd not in commands:
            continue
        for flag, (parents, values) in table.items():
            add(cmd, parents + [flag])                      # a valued flag swallows the first positional here
            for v in (values or []) + (JUNK if values and flag not in LENIENT else []):
                add(cmd, parents + [flag, v])
        for line in lines:
            # "!": the line is the whole command line, positionals included; a list: arguments that hold blanks
            words = line if isinstance(line, list) else line.lstrip("!").split()
            add(cmd, words, positionals=isinstance(line, list) or not line.startswith("!"))
    for a, b in zip(GROUP_BAD, GROUP_BAD[1:] + GROUP_BAD[:1]) if "pileup" in commands else ():
        add("pileup", a.split() + b.split())
        add("pileup", b.split() + a.split())
    return cases


def run_case(exe, cmd, args, prefix):
    """exit code, usage text or None, stderr before it: with the tokens in place of this run's paths"""
    argv = [exe, cmd] + [prefix if a == "PREFIX" else a for a in args]
    r = subprocess.run(argv, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120, cwd=os.path.dirname(prefix))
    assert r.stdout == "", (argv, r.stdout)
    err = r.stderr.replace(prefix, "PREFIX").replace(exe, "EXE").replace(os.path.dirname(os.path.realpath(exe)), "EXEDIR")
    at = err.find("USAGE:")
    return r.returncode, (err[at:] if at >= 0 else None), (err[:at] if at >= 0 else err)


def fold(text, frame):
    """the text with <HEAD> and <TAIL> for the two parts of the command's frame"""
    assert "<HEAD>" not in text and "<TAIL>" not in text
    head, tail = frame
    if text.startswith(head):
        text = "<HEAD>" + text[len(head):]
    if text.endswith(tail):
        text = text[:len(text) - len(tail)] + "<TAIL>"
    return text


def unfold(text, frame):
    return text.replace("<HEAD>", frame[0]).replace("<TAIL>", frame[1])


def record(exe, commands=COMMANDS):
    """the fixture of `commands` as a dict, from the binary `exe`"""
    exe = os.path.abspath(exe)
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "out")
        usage, frames = {}, {}
        for cmd in commands:
            code, text, before = run_case(exe, cmd, ["-h"], prefix)
            assert code == 0 and text and before == "", (cmd, code, before)
            usage[cmd] = text
            code, text, before = run_case(exe, cmd, POSITIONALS[cmd], prefix)
            cut = before.index("output prefix: PREFIX\n") + len("output prefix: PREFIX\n")
            assert code == 1 and text is None
            frames[cmd] = [before[:cut], before[cut:]]
        cases = matrix(commands)
        with ThreadPoolExecutor(8) as pool:
            results = list(pool.map(lambda c: run_case(exe, c[0], c[1], prefix), cases))
        assert not os.listdir(tmp), os.listdir(tmp)           # no case creates a file
    messages = sorted({before for (_, text, before) in results if text is not None})
    rows = {cmd: [] for cmd in commands}
    for (cmd, args), (code, text, before) in zip(cases, results):
        assert text is None or text == usage[cmd], (cmd, args)   # there is one usage text per command
        rows[cmd].append([args, code, int(text is not None), fold(before, frames[cmd]) if text is None else messages.index(before)])
    return {"usage": usage, "frames": frames, "messages": messages, "cases": rows}


def dump(fixture, path):
    with open(path, "w") as f:     # a few cases per line
        f.write("{" + ",\n".join(json.dumps(k) + ": " + json.dumps(fixture[k], indent=1) for k in ("usage", "frames", "messages")))
        f.write(',\n"cases": {')
        for n, cmd in enumerate(fixture["cases"]):
            f.write((",\n" if n else "\n") + json.dumps(cmd) + ": [\n")
            line = ""
            for k, r in enumerate(fixture["cases"][cmd]):
                text = json.dumps(r, separators=(",", ":")) + ("," if k + 1 < len(fixture["cases"][cmd]) else "")
                if line and len(line) + len(text) > 600:
                    f.write(line + "\n")
                    line = ""
                line += text
            f.write(line + "\n]")
        f.write("}}\n")


def load(path=FIXTURE):
    """usage texts by command, and the cases as [(command, arguments, exit code, usage follows, stderr before the usage)]"""
    with open(path) as f:
        fx = json.load(f)
    cases = [(cmd, args, code, usage, fx["messages"][err] if usage else unfold(err, fx["frames"][cmd]))
             for cmd, rows in fx["cases"].items() for args, code, usage, err in rows]
    return fx["usage"], cases


if __name__ == "__main__":
    exe = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
    for path, commands in ((FIXTURE, COMMANDS), (SMOOTH_FIXTURE, SMOOTH_COMMANDS)):
        fixture = record(exe, commands)
        dump(fixture, path)
        n_usage = sum(r[2] for rows in fixture["cases"].values() for r in rows)
        print(f"{os.path.basename(path)}: {sum(map(len, fixture['cases'].values()))} cases, {n_usage} end in the usage text, {os.path.getsize(path)} bytes")

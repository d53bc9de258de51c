"""CPU suite: the argument handling of tools/vre.py.  A usage error -- a missing option, a malformed format, interval or width
string, a count of files that does not fit -- ends with status 2 and the reference's message (ProtocolElGamalRearParser.java,
ProtocolElGamalRearTool.java) before any file or GPU is touched; a missing input ends with status 1.  No GPU: the tool is driven
only as far as its arguments and its input files."""
import os
import subprocess
import sys

from conftest import ROOT

GROUP = ("--bits", "2048")


def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vre.py")] + list(args), capture_output=True, text=True, timeout=120)


def usage_error(message, *args):
    r = run_tool(*args)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-1000:])


def test_usage_errors_carry_the_reference_messages(entry, tmp_path):
    pk, a, b, o1, o2 = (str(tmp_path / n) for n in ("pk", "a", "b", "o1", "o2"))
    # one mode, and -ciphs or -plain behind every mode but -pkeys
    usage_error("exactly one of", *GROUP, pk, a, o1)
    usage_error("exactly one of", "-sub", "-cat", "-ciphs", *GROUP, pk, a, o1)
    usage_error("One of the options \"-plain\" or \"-ciphs\" is required!", "-cat", *GROUP, pk, a, o1)
    usage_error("The options \"-plain\" and \"-ciphs\" can not be combined!", "-cat", "-ciphs", "-plain", *GROUP, pk, a, o1)
    usage_error("Non-positive width! (0)", "-cat", "-ciphs", "-width", "0", *GROUP, pk, a, o1)
    assert run_tool("-cat", "-ciphs", pk, a, o1).returncode == 2                                           # no group
    # -sub
    usage_error("-sub needs -inter", "-sub", "-ciphs", *GROUP, pk, a, o1)
    usage_error("Failed to parse intervals! (3-3) Malformed interval! (3-3)", "-sub", "-inter", "3-3", "-ciphs", *GROUP, pk, a, o1)
    usage_error("No interval is given!", "-sub", "-inter", ":", "-ciphs", *GROUP, pk, a, o1)
    usage_error("Malformed interval! ()", "-sub", "-inter", "0-1::2-3", "-plain", *GROUP, pk, a, o1, o2)
    usage_error("Malformed interval! (2147483648-2147483649)", "-sub", "-inter", "2147483648-2147483649", "-plain", *GROUP, pk, a, o1)
    usage_error("Too few files! (1 < 2)", "-sub", "-inter", "0-3", "-ciphs", *GROUP, pk, a)
    usage_error("Mismatching number of intervals and output filenames! (2 != 1)", "-sub", "-inter", "0-3:3-10", "-ciphs", *GROUP, pk, a, o1)
    # -cat
    usage_error("Too few files! (1)", "-cat", "-ciphs", *GROUP, pk, a)
    # -shallow
    usage_error("-shallow needs -format", "-shallow", "-widths", "2:1", "-ciphs", *GROUP, pk, a, b, o1)
    usage_error("Malformed position string! ((0,))", "-shallow", "-widths", "2:1", "-format", "(0,)", "-ciphs", *GROUP, pk, a, b, o1)
    usage_error("Malformed interval! ( 0)", "-shallow", "-widths", "2:1", "-format", "( 0,0)", "-ciphs", *GROUP, pk, a, b, o1)
    usage_error("Malformed position string! ()", "-shallow", "-widths", "2:1", "-format", "x(0,1)", "-ciphs", *GROUP, pk, a, b, o1)
    usage_error("Non-positive width!", "-shallow", "-widths", "2:0", "-format", "(0,1)", "-ciphs", *GROUP, pk, a, b, o1)
    usage_error("Failed to parse width! (a)", "-shallow", "-widths", "a", "-format", "(0,1)", "-ciphs", *GROUP, pk, a, o1)
    usage_error("The number of widths (2) plus the number of output files (2) specified in the output format does not equal the number "
                "of filenames (3)!", "-shallow", "-widths", "2:1", "-format", "(0,1):(1,0)", "-ciphs", *GROUP, pk, a, b, o1)
    # -deep and -pkeys
    usage_error("-deep needs -noin", "-deep", "-format", "(0,0)", "-plain", *GROUP, pk, a, o1)
    usage_error("Non-positive number of public keys! (0)", "-deep", "-noin", "0", "-format", "(0,0)", "-plain", *GROUP, pk, a, o1)
    usage_error("The number of public keys (2) plus the number of input group element arrays (2) plus the number of output group element "
                "arrays (1) specified in the output format does not equal the number of filenames (4)!",
                "-deep", "-noin", "2", "-format", "(0,0)x(1,0)", "-plain", *GROUP, pk, pk, a, b)
    usage_error("Non-positive number of public keys! (-1)", "-pkeys", "-noin", "-1", "-format", "(0,0)", *GROUP, pk, o1)
    usage_error("There are too few files! (2 < 3)", "-pkeys", "-noin", "2", "-format", "(0,0)x(1,0)", *GROUP, pk, a)
    usage_error("The format and number of output filenames do not match!", "-pkeys", "-noin", "2", "-format", "(0,0)x(1,0)", *GROUP, pk, a, o1, o2)
    usage_error("Malformed interval! (1_0)", "-pkeys", "-noin", "1", "-format", "(1_0,0)", *GROUP, pk, o1)
    assert not any(os.path.exists(p) for p in (pk, a, b, o1, o2))


def test_a_missing_input_is_status_one(entry, tmp_path):
    pk, a, o1, o2 = (str(tmp_path / n) for n in ("pk", "a", "o1", "o2"))
    for args in (("-sub", "-inter", "0-3:3-10", "-ciphs", *GROUP, pk, a, o1, o2),
                 ("-cat", "-plain", "-width", "2", "--curve", "P-256", pk, a, a, o1),
                 ("-shallow", "-widths", "3", "-format", "(0,2):(0,0-2)", "-ciphs", *GROUP, pk, a, o1, o2),
                 ("-deep", "-noin", "1", "-width", "2", "-format", "(0,0)", "-ciphs", *GROUP, pk, a, o1),
                 ("-pkeys", "-noin", "2", "-format", "(0,0)x(1,0)", *GROUP, pk, a, o1)):
        r = run_tool(*args)
        assert r.returncode == 1 and "no such file" in r.stderr, (args, r.returncode, r.stderr[-1000:])            # past the arguments
    assert not any(os.path.exists(p) for p in (o1, o2))

"""`inquistr assoc --firth` above the C ABI, without a GPU: the flag's argument errors (exit status 101, before any device is asked
for), the Python mirror's flag, and the new entry's place in the two ABIs with the new row's documented size and offsets."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")
NAMES = [f"S{i}" for i in range(8)]


@pytest.fixture()
def files(tmp_path):
    rng = np.random.default_rng(3)
    head = "chromosome\tbegin\tend\t" + "\t".join(f"{n}_H{h}" for n in NAMES for h in (1, 2))
    rows = [f"chr1\t{100 * i}\t{100 * i + 20}\t" + "\t".join(str(int(v)) for v in rng.integers(5, 20, 16)) for i in range(5)]
    comb = tmp_path / "c.tsv"
    comb.write_text(head + "\n" + "\n".join(rows) + "\n")
    ph = tmp_path / "p.tsv"
    ph.write_text("individual\tgrp\tage\n" + "".join(f"{n}\t{'Y' if i % 2 else 'N'}\t{30 + i}\n" for i, n in enumerate(NAMES)))
    return comb, ph


def _cli(*args):
    return subprocess.run([CLI, "assoc"] + [str(a) for a in args], capture_output=True, text=True)


def test_firth_argument_errors_are_exit_101(files):
    comb, ph = files
    binary = [comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N,Y"]
    cont = [comb, "--phenocovar", ph, "--phenotype", "age", "--outcome", "continuous"]

    def is_101(r, text):
        return r.returncode == 101 and "panicked" in r.stderr and text in r.stderr and r.stdout == ""

    assert is_101(_cli(*binary, "--firth", "sometimes"), "--firth takes no, fallback or always")
    assert is_101(_cli(*binary, "--firth=yes"), "--firth takes no, fallback or always")
    assert is_101(_cli(*cont, "--firth", "fallback"), "--firth is for --outcome binary")
    assert is_101(_cli(*cont, "--firth", "always"), "--firth is for --outcome binary")
    assert is_101(_cli(*cont, "--firth", "bogus"), "--firth takes no, fallback or always")
    assert _cli(*binary, "--firth").returncode == 2  # a flag without its value is a usage error, as for every other flag
    assert "--firth <no|fallback|always>" in _cli("--help").stdout
    # the accepted values get past the arguments: what stops them here is the missing device (1), or nothing (0)
    for v in ("no", "fallback", "always"):
        r = _cli(*binary, "--firth", v)
        assert r.returncode in (0, 1) and "--firth" not in r.stderr, (v, r.stderr)
    assert _cli(*cont, "--firth", "no").returncode in (0, 1)


def test_python_mirror_takes_the_flag(files):
    comb, ph = files
    for bad in ("sometimes", ""):
        with pytest.raises(call.CallError) as e:
            call.assoc(comb, ph, "grp", "binary", "N,Y", firth=bad)
        assert e.value.status == 101 and "--firth takes" in e.value.message
    with pytest.raises(call.CallError) as e:
        call.assoc(comb, ph, "age", "continuous", firth="always")
    assert e.value.status == 101 and "--outcome binary" in e.value.message
    a = call._assoc_args(comb, ph, "grp", "binary", "N,Y", None, "max", 0.8, None, None, None, False, 0, "fallback")
    assert (a.firth, a.reserved, a.device) == (1, 0, 0) and call.ASSOC_FIRTH == {"no": 0, "fallback": 1, "always": 2}
    assert call._assoc_args(comb, ph, "grp", "binary", "N,Y", None, "max", 0.8, None, None, None, False, 0).firth == 0
    # the samples entry reads the same struct and does not mind the flag
    assert call.assoc_samples(comb, ph, "grp", "binary", "N,Y")[0] == NAMES


def test_new_entry_in_both_abis():
    D = hipcall.load()
    assert "inq_assoc_rows_firth" in hipcall.ABI_SYMBOLS and hasattr(D, "inq_assoc_rows_firth") and len(D.inq_assoc_rows_firth.argtypes) == 12
    assert D.inq_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "inquistr_hip.h")).read()
    m = re.search(r"inq_assoc_firth_row_t is (\d+) bytes: ([^.]*)\.", hdr)
    assert m and int(m.group(1)) == 56 == C.sizeof(hipcall.AssocFirthRowC) == hipcall.ASSOC_FIRTH_ROW_DTYPE.itemsize
    stated = {name: int(off) for name, off in re.findall(r"([a-z_0-9]+) (\d+)", m.group(2).replace("\n", " ").replace("*", " "))}
    assert stated == {f: getattr(hipcall.AssocFirthRowC, f).offset for f, _ in hipcall.AssocFirthRowC._fields_}
    assert stated == {f: hipcall.ASSOC_FIRTH_ROW_DTYPE.fields[f][1] for f in hipcall.ASSOC_FIRTH_ROW_DTYPE.names}
    for name, val in hipcall.ASSOC_FIRTH_WHEN.items():
        assert re.search(rf"#define INQ_ASSOC_FIRTH_{name.upper()} {val}\b", hdr), name
    for val, name in enumerate(hipcall.ASSOC_FIRTH_STATUS):
        assert re.search(rf"#define INQ_ASSOC_FIRTH_ROW_{name} {val}\b", hdr), name
    # the ordinary row is what it was
    assert C.sizeof(hipcall.AssocRowC) == 88
    # the host's argument struct: the new field behind the old ones, which keep their offsets
    host = open(os.path.join(ROOT, "include", "inquistr_host.h")).read()
    body = re.search(r"typedef struct inq_assoc_args \{(.*?)\} inq_assoc_args_t;", host, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields[-2:] == ["firth", "reserved"] and fields[:-2] == [f for f, _ in call.AssocArgsC._fields_]
    assert call.AssocArgsFirthC.firth.offset == C.sizeof(call.AssocArgsC) == 88 and C.sizeof(call.AssocArgsFirthC) == 96
    for name, val in (("NO", 0), ("FALLBACK", 1), ("ALWAYS", 2)):
        assert re.search(rf"#define INQ_HOST_FIRTH_{name} {val}\b", host), name
    # a bad `when` is refused before a context is looked at
    assert D.inq_assoc_rows_firth(None, None, 0, 0, None, None, 0, 0, 0.8, 0, None, None) == hipcall.INQ_ERR_ARG

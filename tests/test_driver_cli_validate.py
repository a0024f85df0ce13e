"""`mtb_classify --validate-db` on the command line, before any GPU work (metabuli_amd/csrc/host/classify_main.cpp, host/audit_plan.h):
with 1 the files of the database are checked first, with the reference's messages, and a missing one ends the run before a device is
touched; with 0 the flag is still the compatibility no-op it was.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metabuli_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(os.path.join(CSRC, "libmtb.so")):
        pytest.skip("libmtb.so not built")
    subprocess.check_call(["make", "-C", CSRC, "mtb_classify"], stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "mtb_classify")


def _run(exe, *args):
    p = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return p.returncode, p.stdout, p.stderr


def _db(d, without=()):
    os.makedirs(os.path.join(d, "taxonomy"))
    for f in ("diffIdx", "info", "split", "taxID_list", "db.parameters", "taxonomy/nodes.dmp", "taxonomy/names.dmp", "taxonomy/merged.dmp"):
        if f not in without:
            open(os.path.join(d, f), "wb").write(b"\x00" * 8)
    return str(d)


def test_missing_diffidx_ends_the_run_before_any_device_work(exe, tmp_path):
    d = _db(tmp_path / "db", without=("diffIdx",))
    rc, out, err = _run(exe, "--validate-db", "1", "--seq-mode", "1", "r.fq", d, str(tmp_path), "job")
    assert rc == 1
    assert out.splitlines()[:2] == ["Validating database: " + d, "Check if required files exist..."]
    assert 'Error: "diffIdx" file is missing in the database directory.' in err and "Database validation failed." in err
    assert "All required files are present." not in out
    assert "HIP" not in err and "device" not in err.lower() and "accepted for compatibility" not in err      # no context was created, the flag is no no-op
    assert not os.path.exists(tmp_path / "job_classifications.tsv")


def test_file_checks_follow_the_reference(exe, tmp_path):
    d = _db(tmp_path / "db", without=("info", "taxID_list", "taxonomy/names.dmp"))
    rc, out, err = _run(exe, "--validate-db", "1", "--seq-mode", "1", "r.fq", d, str(tmp_path), "job")
    assert rc == 1
    for msg in ('Error: "info" file is missing in the database directory.', 'Error: "taxID_list" file is missing in the database directory.',
                'Error: "names.dmp" file is missing in the "DBDIR/taxonomy" directory.', "Please check the database directory and make sure all required files are present."):
        assert msg in err, err
    assert '"split" file is missing' not in err
    d2 = _db(tmp_path / "db2")
    open(os.path.join(d2, "diffIdx"), "wb").close()
    rc, out, err = _run(exe, "--validate-db", "1", "--seq-mode", "1", "r.fq", d2, str(tmp_path), "job")
    assert rc == 1 and "All required files are present." in out and "Error: diffIdx file is empty." in err      # (the size checks follow the presence checks)
    open(os.path.join(d2, "diffIdx"), "wb").write(b"\x00" * 7)
    rc, out, err = _run(exe, "--validate-db", "1", "--seq-mode", "1", "r.fq", d2, str(tmp_path), "job")
    assert rc == 1 and "Error: diffIdx file size is not a multiple of 2." in err


def test_validate_db_0_is_still_the_compatibility_note(exe, tmp_path):
    rc, out, err = _run(exe, "--validate-db", "0", "--seq-mode", "1", "r.fq", str(tmp_path / "nodb"), str(tmp_path), "job")
    assert rc == 1
    assert err.count("mtb_classify: --validate-db 0 accepted for compatibility with `metabuli classify`, it has no effect here") == 1
    assert "Validating database" not in out

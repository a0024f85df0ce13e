"""`mtb_classify --kmer-coverage` around an engine WITHOUT the coverage entry points: the driver linked against
tests/null_engine/null_mtb.cpp exactly as tests/test_driver_null_engine.py links it (its fixtures are taken from there).  The driver
references mtb_index_coverage_* weakly: it must link, run unchanged without the flag, and refuse the flag in one line."""
import os

from test_driver_null_engine import expected_files, make_reads, null_db, null_driver, run, same_report, write_fastq  # noqa: F401  (fixtures)


def _inputs(tmp_path, n=300):
    names = [f"read{i}" for i in range(n)]
    r1 = make_reads(n, 31)
    fq = str(tmp_path / "r.fq")
    write_fastq(fq, names, r1)
    return names, r1, fq


def test_flag_is_refused_where_the_engine_has_no_coverage(null_driver, null_db, tmp_path):
    d, tax, ids = null_db
    _, _, fq = _inputs(tmp_path)
    p = run(null_driver, ["--seq-mode", "1", "--kmer-coverage", "1", fq, d, str(tmp_path), "job"], check=False)
    assert p.returncode == 1
    assert p.stderr.decode() == "mtb_classify: --kmer-coverage 1: this engine has no k-mer coverage support\n"
    assert p.stdout == b"" and not any(f.startswith("job_") for f in os.listdir(tmp_path))       # refused before anything is opened or written


def test_without_the_flag_nothing_changes(null_driver, null_db, tmp_path):
    d, tax, ids = null_db
    names, r1, fq = _inputs(tmp_path)
    want_c, want_r, _, _, _ = expected_files(str(tmp_path), tax, ids, names, r1, None)
    for extra in ([], ["--kmer-coverage", "0"]):
        out = tmp_path / ("out%d" % len(extra))
        out.mkdir()
        run(null_driver, ["--seq-mode", "1", "--max-reads", "97"] + extra + [fq, d, str(out), "job"])
        assert open(out / "job_classifications.tsv").read() == want_c
        assert same_report(open(out / "job_report.tsv").read(), want_r)
        assert sorted(os.listdir(out)) == ["job_classifications.tsv", "job_krona.html", "job_report.tsv"]


def test_flag_is_refused_next_to_partitioned_and_filter(null_driver, null_db, tmp_path):
    d, tax, ids = null_db
    _, _, fq = _inputs(tmp_path)
    before = sorted(os.listdir(tmp_path))
    for args in (["--seq-mode", "1", "--kmer-coverage", "1", "--partitioned", "1", "--devices", "0,1", fq, d, str(tmp_path), "job"],
                 ["--seq-mode", "1", "--filter", "1", "--kmer-coverage", "1", fq, d]):
        p = run(null_driver, args, check=False)
        assert p.returncode == 1
        assert p.stderr.decode() == "mtb_classify: --kmer-coverage 1 cannot be combined with --partitioned 1 or --filter 1\n"
        assert sorted(os.listdir(tmp_path)) == before
    # the same combinations with the flag off run as they always did
    run(null_driver, ["--seq-mode", "1", "--kmer-coverage", "0", "--filter", "1", fq, d])
    assert os.path.exists(str(tmp_path / "r_filtered.fna"))

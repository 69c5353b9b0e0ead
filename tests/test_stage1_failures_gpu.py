"""bdg_stage1_run's ways out after a failure: an input, a TSV or a trimmed file that cannot be opened, a chunk that fails while
others are in flight, one that fails in the final drain, and a run that fails its last check.  Each returns its code and message,
and leaves the two contexts as it found them: the run with every output and the plain run that follow write the bytes and count
the numbers they did before.  Five chunks of 300 reads over two contexts with two slots each: the collect inside the loop and
the drain behind it both run.  Text and integers: every comparison is exact."""
import numpy as np
import pytest

from badger_amd import _native, synth

pytestmark = pytest.mark.gpu

N, W, CHUNK = 1500, 2000, 300
PLAIN_HEADER = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end"
HEADER = PLAIN_HEADER + "\twhitelist_barcode\twhitelist_dist\twhitelist_ties\twhitelist_candidates"


def _counts(res):
    return {f: getattr(res, f) for cls in type(res).__mro__ for f, _ in cls.__dict__.get("_fields_", ()) if not f.startswith("seconds_")}


class _Runs:
    def __init__(self, tmp):
        self.tmp, self.k = tmp, 0
        wl = synth.make_whitelist(W)
        b, o = synth.make_reads(N, wl, seed=151, tso=True)
        self.fa = str(tmp / "reads.fa")
        with open(self.fa, "w") as f:
            f.write("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(synth.reads_to_list(b, o))))
        self.ctxs = [_native.Context(0), _native.Context(0)]
        for c in self.ctxs:
            c.whitelist_load(wl)

    def path(self, name):
        self.k += 1
        return str(self.tmp / ("%d_%s" % (self.k, name)))

    def run(self, in_path=None, out=None, header=PLAIN_HEADER, **kw):
        return _native.stage1_run(self.ctxs, in_path or self.fa, out or self.path("out.tsv"), header, 12, threads=1, chunk_reads=CHUNK, **kw)

    def full(self, **kw):
        """whitelist with candidates, correction, trimming, chimera cuts -> (counters, the three files)"""
        p = dict(out=self.path("full.tsv"), corrected_path=self.path("full.corr"), trimmed_path=self.path("full.fa"))
        p.update(kw)
        res = self.run(header=HEADER, whitelist=True, max_bc_dist=2, bc_candidates=3, chimera_max_ed=3, **p)
        assert isinstance(res, _native.Stage1ResultChimera)
        return _counts(res), [open(p[k], "rb").read() for k in ("out", "corrected_path", "trimmed_path")]

    def plain(self):
        out = self.path("plain.tsv")
        res = self.run(out=out)
        assert type(res) is _native.Stage1Result
        return _counts(res), open(out, "rb").read()

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the two contexts, and what the full and the plain run give on them before anything has failed (read only)"""
    R = _Runs(tmp_path_factory.mktemp("stage1_failures"))
    R.full0, R.plain0 = R.full(), R.plain()
    yield R
    R.close()


def test_reference_runs(runs):
    counts, files = runs.full0
    assert counts["reads"] == N and counts["chunks"] == 5                  # (one more than the four in flight)
    assert counts["whitelist_barcodes"] > 0 and counts["whitelist_corrected"] > 0 and counts["trimmed_reads"] > 0 and counts["trimmed_tso"] > 0
    assert all(len(f) > 0 for f in files)
    counts, tsv = runs.plain0
    assert counts["reads"] == N and counts["chunks"] == 5 and counts["out_bytes"] == len(tsv) - len(PLAIN_HEADER) - 1


def _tags(n):
    return dict(cell_rank=np.zeros(n, np.uint32), cell_has=np.ones(n, np.uint8))


# name -> (the failing run, its code, what its message says)
FAILURES = {
    "no_input": (lambda R: R.full(in_path=str(R.tmp / "nowhere" / "reads.fa")), _native.E_ARG,
                 lambda R: "cannot read %s (unknown extension or unreadable file)" % (R.tmp / "nowhere" / "reads.fa")),
    "no_out_dir": (lambda R: R.run(out=str(R.tmp / "nowhere" / "out.tsv"), header=HEADER, whitelist=True, corrected_path=R.path("x.corr")),
                   _native.E_ARG, lambda R: "cannot write %s" % (R.tmp / "nowhere" / "out.tsv")),
    "no_trimmed_dir": (lambda R: R.run(header=HEADER, whitelist=True, corrected_path=R.path("x.corr"),
                                       trimmed_path=str(R.tmp / "nowhere" / "x.fa")),
                       _native.E_ARG, lambda R: "cannot write %s" % (R.tmp / "nowhere" / "x.fa")),
    # the first chunk is collected inside the loop, with the others in flight
    "tags_200": (lambda R: R.run(trimmed_path=R.path("t.fa"), tags=_tags(200)), _native.E_ARG,
                 lambda R: "the input holds more reads than the 200 the tag arrays hold"),
    # the fourth chunk is collected in the final drain
    "tags_1000": (lambda R: R.run(trimmed_path=R.path("t.fa"), tags=_tags(1000)), _native.E_ARG,
                  lambda R: "the input holds more reads than the 1000 the tag arrays hold"),
    # every chunk goes through; the count behind the loop fails
    "tags_2000": (lambda R: R.run(trimmed_path=R.path("t.fa"), tags=_tags(2000)), _native.E_ARG,
                  lambda R: "the input holds %d reads, the tag arrays 2000" % N),
}


@pytest.mark.parametrize("name", list(FAILURES))
def test_failure_leaves_the_contexts_as_they_were(runs, name):
    fail, code, message = FAILURES[name]
    with pytest.raises(_native.BadgerHipError) as e:
        fail(runs)
    assert e.value.code == code
    assert str(e.value) == "libbadger_hip error %d: %s" % (code, message(runs))
    counts, files = runs.full()
    assert files == runs.full0[1]
    assert counts == runs.full0[0]
    # (trimming and the chimera search are off again on the contexts)
    assert runs.plain() == runs.plain0

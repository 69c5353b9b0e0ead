"""--molecule_consensus on the GPU, in a 3' and a 5' mode: the consensus file equals the rule of badger_amd/consensus.py applied to
the tagged file the same run wrote, byte for byte; every other output and the printed count are what a run without the flag
gives; `python -m badger_amd.consensus` on that tagged file writes the same bytes.  About 3,000 synthetic reads: 1,200 of a few
dozen cells plus siblings of them - the same read with new sequencing errors in the middle of its cDNA, so that it keeps its
barcode and UMI and the molecules hold several different reads."""
import io
import logging
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import consensus_cases as cc
from badger_amd import badger, common, synth
from badger_amd import consensus as cs

pytestmark = pytest.mark.gpu

N_CELLS = 40
MODES = {"tenX_v3": (12, cs.ANCHOR_END), "tenX_5p_v2": (10, cs.ANCHOR_START)}


class _Messages(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _stage2(argv):
    """-> (what the run printed, its log messages)"""
    buf, seen = io.StringIO(), _Messages()
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with redirect_stdout(buf):
            badger.main(argv)
    finally:
        log.removeHandler(seen)
    return buf.getvalue(), seen.lines


@pytest.fixture(scope="module", params=sorted(MODES))
def run(request, tmp_path_factory):
    mode = request.param
    umi_len, anchor = MODES[mode]
    tmp = tmp_path_factory.mktemp("cons_" + mode)
    wl = synth.make_whitelist(400)
    if mode.startswith("tenX_5p"):
        b, o = synth.make_reads_5p(1200, wl, seed=5, umi_len=umi_len, n_cells=N_CELLS)
        text = np.asarray(b).tobytes().decode()
        base = [text[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]
    else:
        b, o = synth.make_reads(1200, wl, seed=5, umi_len=umi_len, n_cells=N_CELLS, tso=True)
        base = synth.reads_to_list(b, o)
    rng = np.random.default_rng(6)
    reads = list(base)
    for i in range(len(base)):                                       # 0 .. 4 siblings: new errors between the ends, which stay
        x = base[i]
        if len(x) < 420:
            continue
        for _ in range(int(rng.integers(0, 5))):
            reads.append(x[:160] + cc.mutate(rng, x[160:-160]) + x[-160:])
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    args = ["-r", fq, "-d", mode, "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup"]
    plain, with_flag = str(tmp / "plain"), str(tmp / "cons")
    out_plain = _stage2(args + ["-o", plain, "--tagged_reads", plain + ".fa"])
    out_flag = _stage2(args + ["-o", with_flag, "--tagged_reads", with_flag + ".fa", "--molecule_consensus", with_flag + ".consensus.fa"])
    return dict(mode=mode, anchor=anchor, tmp=tmp, args=args, plain=plain, cons=with_flag, out_plain=out_plain, out_flag=out_flag, n=len(reads))


def test_consensus_file_is_the_rule_over_the_tagged_file(run):
    tagged = open(run["cons"] + ".fa", "rb").read()
    want, counts = cs.consensus_text(tagged, run["anchor"], 3, 20, cs.consensus_groups)
    got = open(run["cons"] + ".consensus.fa", "rb").read()
    assert got == want
    # the input is what the test is for: molecules of several reads, most of whose members vote, and bases that change
    assert counts["molecules"] > 200 and counts["voted"] > 60 and counts["accepted"] > 150
    assert got.count(b">") == counts["molecules"] and got.count(b"\tCN:i:1\n") + got.count(b"\tCN:i:1\t") == counts["molecules"] - counts["voted"]
    backbone = dict(zip(*[iter(tagged.split(b"\n")[:-1])] * 2))
    pairs = list(zip(*[iter(got.split(b"\n")[:-1])] * 2))
    changed = sum(1 for h, seq in pairs if backbone[re.sub(rb"\tCN:i:\d+", b"", h)] != seq)
    print("molecules %d, with a vote %d, members accepted %d, consensus differs from the backbone in %d" % (
        counts["molecules"], counts["voted"], counts["accepted"], changed))
    assert changed > 30
    line = "Consensus: %d molecules to %s, %d with a vote; members: %d accepted, rejected %d by distance, %d by band, %d by length" % (
        counts["molecules"], run["cons"] + ".consensus.fa", counts["voted"], counts["accepted"], counts["rej_dist"], counts["rej_band"], counts["rej_len"])
    assert any(line in m for m in run["out_flag"][1]), run["out_flag"][1][-3:]


def test_nothing_else_moves(run):
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert open(run["cons"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    # but for the consensus line the run logged what it logs without the flag
    logged = [m.replace(run["cons"], run["plain"]) for m in run["out_flag"][1] if "Consensus: " not in m]
    assert logged == run["out_plain"][1] and len(logged) + 1 == len(run["out_flag"][1])


def test_stand_alone_module_writes_the_same_bytes(run, caplog):
    out = str(run["tmp"] / "alone.fa")
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        cs.main(["-i", run["cons"] + ".fa", "-o", out, "--anchor", "end" if run["anchor"] == cs.ANCHOR_END else "start"])
    assert open(out, "rb").read() == open(run["cons"] + ".consensus.fa", "rb").read()
    assert any("Consensus: " in r.getMessage() for r in caplog.records)
    # other values reach the device: at 2 reads more molecules vote, at 0 % only identical reads do
    tagged = open(run["cons"] + ".fa", "rb").read()
    for min_reads, pct in ((2, 20), (3, 0)):
        cs.main(["-i", run["cons"] + ".fa", "-o", out, "--anchor", "end" if run["anchor"] == cs.ANCHOR_END else "start",
                 "--consensus_min_reads", str(min_reads), "--consensus_max_ed", str(pct)])
        want, counts = cs.consensus_text(tagged, run["anchor"], min_reads, pct, cs.consensus_groups)
        assert open(out, "rb").read() == want

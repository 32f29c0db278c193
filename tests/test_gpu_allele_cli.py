"""-m gpu: --alleles on the command line.  The catalogue of tests/allele_cases.py as BAM, plain SAM and BGZF SAM with a VCF of its sites
gives the allele_counts.tsv of the Python restatement of the contract (tests/allele_ref.py), byte for byte, and leaves every other report
file as a run without the flag writes it; the same file comes out under RSQC_DECODE=host and with --sort on a shuffled copy; a cohort of
two samples whose headers order the contigs differently gives each its own file; a malformed or unopenable site file ends the run."""
import gzip
import os
import random
import subprocess

import pytest

from rnaseqc_amd import bamio, synth
from tests import allele_cases as ac
from tests import allele_ref as ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu

Q, BQ = ac.MIN_MAPQ, ac.MIN_BASEQ


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("allelefiles")
    f = Case()
    f.dir = d
    ann = synth.make_annotation(seed=63, contigs=[("chrA", 21001, 0), ("chrB", 1003, 0), ("chrC", 500, 0), ("chrD", 500_000, 30)])
    f.paths = {k: str(d / v) for k, v in dict(gtf="a.gtf", vcf="sites.vcf.gz", bam="c.bam", sam="c.sam", bgzf="c.sam.gz", shuffled="shuffled.bam", other="other.bam", lst="cohort.txt",
                                              bad="bad.vcf").items()}
    bamio.write_gtf(f.paths["gtf"], ann)
    # the VCF: the catalogue's sites in a shuffled order, with a repeated line, an indel, a contig no header has
    body = ac.vcf_text(ac.SITES).splitlines()
    head, lines = body[:2], body[2:]
    random.Random(4).shuffle(lines)
    lines += [lines[5].replace("\trs", "\tagain"), "chrA\t1200\tindel\tAC\tA", "chrUn\t5\tnowhere\tA\tC"]
    f.vcf_text = "\n".join(head + lines) + "\n"
    with open(f.paths["vcf"], "wb") as out:
        out.write(gzip.compress(f.vcf_text.encode()))
    f.lines, f.skipped = ref.parse_sites(f.vcf_text)
    f.records = ac.in_coordinate_order(ac.catalogue())                # (without the BAM-only records: an operation code above 8 ends a run)
    ac.write_bam(f.paths["bam"], f.records, block=4099)
    ac.write_sam(f.paths["sam"], f.records)
    ac.write_sam(f.paths["bgzf"], f.records, bgzf=True, block=5003)
    order = list(range(len(f.records)))
    random.Random(5).shuffle(order)
    ac.write_bam(f.paths["shuffled"], [f.records[k] for k in order])
    # a second sample: the same alignments under a header that orders the contigs differently
    f.other_contigs = [ac.CONTIGS[k] for k in (3, 0, 2, 1)]
    to = {3: 0, 0: 1, 2: 2, 1: 3}
    f.other_records = ac.in_coordinate_order([r[:4] + (to[r[4]],) + r[5:] for r in f.records])
    ac.write_bam(f.paths["other"], f.other_records, contigs=f.other_contigs)
    f.common = ["--alleles=" + f.paths["vcf"], "--allele-mapq=%d" % Q, "--allele-baseq=%d" % BQ]
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, [f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    return f


def _want(f, names, records):
    sites, meta, off, dup = ref.resolve_sites(f.lines, names)
    counts, info = ref.tables(records, len(names), sites, Q, BQ)
    return ref.format_file(names, sites, meta, counts).encode(), info, off, dup


def test_alleles_on_the_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, [*files.common, files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))
    assert rc == 0, se
    text, i, off, dup = _want(files, ac.NAMES, files.records)
    assert (off, dup, files.skipped) == (1, 1, 1) and i["n_sites"] == len(ac.SITES) and i["observations"] > 3000
    got, want = _reports(out), _reports(files.plain_out)
    assert got["x.allele_counts.tsv"] == text
    assert sorted(got) == sorted(list(want) + ["x.allele_counts.tsv"]) and len(want) >= 5
    for name in want:
        assert got[name] == want[name], name                          # every other report file: what a run without the flag writes
    assert ("Alleles: sites %d, skipped_lines 1, off_header_lines 1, duplicate_lines 1, records %d, hit_records %d, observations %d, off_contig %d, low_mapq %d, no_seq %d, "
            "inconsistent %d, no_qual %d, alleles_ms " % (i["n_sites"], i["records"], i["hit_records"], i["observations"], i["off_contig_records"], i["low_mapq_records"],
                                                          i["no_seq_records"], i["inconsistent_records"], i["no_qual_records"])) in so, so


@pytest.mark.parametrize("kind,args,env", [("bam", [], dict(RSQC_DECODE="host", RSQC_BATCH="70")), ("sam", [], dict(RSQC_SAM_CHUNK="50000")), ("bgzf", [], {}), ("bam", [], dict(RSQC_ALLELE_MERGE="1")), ("sam", [], dict(RSQC_ALLELE_MERGE="0")),
                                           ("shuffled", ["--sort"], {}), ("bam", ["--cycles", "--junctions", "--bedgraph", "--gene-body", "--tin", "--mark-duplicates"], {})],
                         ids=["host_decode", "plain_sam", "bgzf_sam", "bam_merged", "sam_not_merged", "sort_shuffled", "with_the_other_extensions"])
def test_the_same_file_on_other_routes(cli, files, kind, args, env):
    out = str(files.dir / ("route_" + kind + "_".join(a.strip("-") for a in args) + ("_host" if env.get("RSQC_DECODE") else "") + env.get("RSQC_ALLELE_MERGE", "")))
    rc, so, se = _run(cli, [*files.common, *args, files.paths["gtf"], files.paths[kind], out, "-s", "x", "-v"], env=env)
    assert rc == 0, se
    text, i, _, _ = _want(files, ac.NAMES, files.records)
    assert _reports(out)["x.allele_counts.tsv"] == text
    assert "Alleles: sites %d," % i["n_sites"] in so and ", observations %d," % i["observations"] in so


def test_cohort_of_two_samples_with_differently_ordered_headers(cli, files):
    """The site file is resolved against each sample's header; a missing sample between them gets no file."""
    with open(files.paths["lst"], "w") as f:
        f.write("%s\tfirst\n%s\tgone\n%s\tsecond\n" % (files.paths["bam"], str(files.dir / "missing.bam"), files.paths["other"]))
    out = str(files.dir / "cohort")
    rc, so, se = _run(cli, [*files.common, "--bam-list", files.paths["lst"], files.paths["gtf"], out, "-v"])
    assert rc == 10, (rc, se)
    got = _reports(out)
    first, second = _want(files, ac.NAMES, files.records)[0], _want(files, [c[0] for c in files.other_contigs], files.other_records)[0]
    assert got["first.allele_counts.tsv"] == first and got["second.allele_counts.tsv"] == second
    assert first != second and sorted(first.splitlines()) == sorted(second.splitlines())      # (the same rows in another contig order)
    assert not [n for n in got if n.startswith("gone.")] and so.count("Alleles: sites ") == 2


def test_a_malformed_and_an_unopenable_site_file(cli, files):
    with open(files.paths["bad"], "w") as f:
        f.write("#x\nchrA\t5\t.\tA\tC\nchrA\tfive\t.\tA\tC\n")
    out = str(files.dir / "bad_out")
    rc, so, se = _run(cli, ["--alleles", files.paths["bad"], files.paths["gtf"], files.paths["bam"], out, "-s", "x"])
    assert rc == 11 and "Failed to parse the sites: %s:3: " % files.paths["bad"] in se, (rc, se)
    rc, so, se = _run(cli, ["--alleles", str(files.dir / "none.vcf"), files.paths["gtf"], files.paths["bam"], out, "-s", "x"])
    assert rc == 10 and "none.vcf" in se, (rc, se)
    assert not os.path.exists(out) or not os.listdir(out)

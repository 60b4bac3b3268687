"""The SAM parser's records through the product. The good records of tests/sam_cases.py on selected chromosomes, written
as one SAM file and as one .sam.gz and split into a single cluster, come out as the bytes tests/sam_ref.py gives for
them, whatever the size of the ranges the text is cut into; and each of the parser's error codes reaches the caller as
the phrase of ``sam_what`` in bam_input.cpp with the line's number.

The expected file is built from the restatement's records, not from ``se.source_of_recs``: most lines of the table
(``-0``, lower-case bases, the float texts) are not what tests/sam_writer.py would write for any ``bw.Rec``. Where a
line is made of a ``bw.Rec``, tests/test_sam_parse_cpu.py holds the restatement to ``bw.encode_record``."""
import os

import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_writer as bw
from tests import sam_cases as sc
from tests import sam_ref as sr
from tests import sam_writer as sw
from tests import split_expected as se
from tests.test_gpu_split_clusters import check_outputs

pytestmark = pytest.mark.gpu

# sam_what of bam_input.cpp, by SamErr
PHRASES = {
    sr.FIELDS: "does not have 11 non-empty tab-separated mandatory fields",
    sr.NAME: "has a QNAME longer than 254 characters",
    sr.FLAG: "has a FLAG that is not an integer in [0, 65535]",
    sr.RNAME: "has an RNAME that no @SQ line names",
    sr.POS: "has a POS that is not an integer in [0, 2^31 - 1]",
    sr.MAPQ: "has a MAPQ that is not an integer in [0, 255]",
    sr.CIGAR: "has a malformed CIGAR",
    sr.RNEXT: "has an RNEXT that is not '*', '=' or an @SQ name",
    sr.PNEXT: "has a PNEXT that is not an integer in [0, 2^31 - 1]",
    sr.TLEN: "has a TLEN that is not an integer in [-(2^31 - 1), 2^31 - 1]",
    sr.QUAL: "has a QUAL that is not '*', not as long as SEQ or not in '!'..'~'",
    sr.CIGAR_SEQ: "has CIGAR and SEQ lengths that differ",
    sr.AUX: "has a malformed optional field",
    sr.HEADER: "is a header line after the first alignment line",
    sr.EMPTY: "is empty",
    sr.MANY_OPS: "has more than 65535 CIGAR ops",
}
HEADER = sw.header_text(sc.REFS).encode()


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    """The SAM file, its .sam.gz and the expected cluster file."""
    d = tmp_path_factory.mktemp("sam_records")
    lines = sc.product_lines()
    records = [sr.parse_line(ln.decode("latin-1"), sc.NAMES) for ln in lines]
    keys = [se.ref_pos(r) for r in records]
    assert keys == sorted(keys) and len(records) > 150 and {k[0] for k in keys} == {0, 1}
    assert max(len(r) for r in records) > se.CUT  # the record of 65535 ops spans BGZF members
    text = HEADER + sc.text_of(lines)
    sam, gz = str(d / "table.sam"), str(d / "table.sam.gz")
    open(sam, "wb").write(text)
    open(gz, "wb").write(bw.bgzf(text))
    assert HEADER.decode() == se.default_text(sc.REFS)
    expected, dropped = se.expected_files([se.Source(HEADER.decode(), sc.REFS, records)], [0], [0, 1], d)
    assert dropped == 0
    return dict(sam=sam, gz=gz, expected=expected, n=len(records))


@pytest.mark.parametrize("batch", [None, "64", "1"])
@pytest.mark.parametrize("kind", ["sam", "gz"])
def test_split_writes_the_restatements_records(product, tmp_path, monkeypatch, kind, batch):
    """SECEDO_BAM_BATCH_BYTES unset, at 64 and at 1, where every line is a range of its own."""
    if batch is None:
        monkeypatch.delenv("SECEDO_BAM_BATCH_BYTES", raising=False)
    else:
        monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", batch)
    info = secedo_amd.split_clusters([product[kind]], [0], tmp_path, [0, 1])
    check_outputs(tmp_path, product["expected"])
    assert (info["records"], info["dropped_records"]) == (product["n"], 0)


def first_error_lines():
    seen = {}
    for code, what, ln in sc.error_lines():
        seen.setdefault(code, (what, ln))
    assert sorted(seen) == list(range(1, 17))
    return [pytest.param(code, ln, id="code_%d" % code) for code, (what, ln) in sorted(seen.items())]


@pytest.mark.parametrize("code,bad", first_error_lines())
def test_error_messages_name_the_defect_and_the_line(tmp_path, code, bad):
    path = tmp_path / "bad.sam"
    path.write_bytes(HEADER + sc.text_of([sc.GOOD, bad, sc.GOOD]))
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([str(path)], None, False, 0, 100, 0, 0, 0, 1, 0)
    line_no = HEADER.count(b"\n") + 2
    assert ("file 0 (%s), line %d %s" % (path, line_no, PHRASES[code])) in str(e.value), str(e.value)
    limit = code == sr.MANY_OPS  # codes 16 and 17 are SECEDO_E_LIMIT; 17 needs a 2 GiB record
    assert e.value.code == (secedo_amd._lib.E_LIMIT if limit else secedo_amd._lib.E_INVALID_ARG)
    assert os.listdir(str(tmp_path)) == ["bad.sam"]

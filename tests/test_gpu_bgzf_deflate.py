"""The BGZF encoder on the GPU (secedo_amd.bgzf_deflate, bgzf_deflate_kernels.hip): the inputs and checks of
tests/test_bgzf_deflate_cpu.py, and byte for byte the output of the host program built from the same header, which is
what catches a race between lanes. Our own decoder (secedo_amd.bgzf_inflate) reads every file back."""
import numpy as np
import pytest

import secedo_amd
from secedo_amd import variant
from tests import bgzf_deflate_cases as dc

pytestmark = pytest.mark.gpu

CASES = dc.cases()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deflate_host")
    return {name: dc.host_encode(data, tmp, name) for name, data in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_and_zlib_reads_it(host, tmp_path, name):
    data = CASES[name]
    raw = secedo_amd.bgzf_deflate(data)
    dc.check_file(raw, data)
    assert raw == host[name]
    assert secedo_amd.bgzf_deflate(data) == raw  # two runs give the same bytes
    path = tmp_path / "x.gz"
    path.write_bytes(raw)
    assert secedo_amd.bgzf_inflate(str(path)).tobytes() == data  # our own decoder accepts our own encoder


def test_stats_of_a_call():
    data = CASES["sam_%d" % (2 * dc.CUT + 1)] + CASES["random_65280"]
    raw = secedo_amd.bgzf_deflate(data)
    st = variant.vcf_stats()
    assert st["output"] == "bgzf" and st["files"] == 1 and st["text_bytes"] == len(data)
    assert st["compressed_bytes"] == len(raw) and st["blocks"] == 4 and st["stored_blocks"] == 1


def test_one_launch_with_300_tiny_inputs(host, tmp_path):
    rng = np.random.default_rng(23)
    sam = dc.gw.sam_like_text(40)
    inputs = []
    for k in range(300):
        n = 0 if k % 7 == 0 else int(rng.integers(1, 400))
        o = int(rng.integers(0, len(sam) - 400))
        inputs.append(sam[o:o + n])
    inputs[5] = CASES["sam_%d" % (dc.CUT + 1)]  # one input of two members among them
    files = variant.bgzf_deflate_many(inputs)
    st = variant.vcf_stats()
    assert len(files) == 300 and st["files"] == 300
    assert st["blocks"] == sum(-(-len(d) // dc.CUT) for d in inputs) and st["compressed_bytes"] == sum(map(len, files))
    for k, (raw, data) in enumerate(zip(files, inputs)):
        dc.check_file(raw, data, with_tokens=k < 20)
        if not data:
            assert raw == dc.gw.EOF_MEMBER
    assert files[5] == host["sam_%d" % (dc.CUT + 1)]
    for k in (1, 2, 3, 150, 299):  # the batch gives what a launch of its own gives
        assert files[k] == secedo_amd.bgzf_deflate(inputs[k]), k
    assert files[1] == dc.host_encode(inputs[1], tmp_path, "tiny")


# ---- the slice borders of the encoder's driver (bgzf_encoder.cpp), reached through SECEDO_BGZF_SLICE_MEMBERS

def _border_inputs():
    """Eight files of 0, 1, 0xFF00, 2 * 0xFF00 + 1, 5, 0, 0 and 0xFF00 + 1 bytes: 8 members. The one of 0xFF00 bytes
    is random (a stored member), the rest SAM-like text. In this order 6 members lie in front of the two empty files,
    so their EOF members follow a slice's last member at 1, 2 and 3 members per slice."""
    sam = CASES["sam_%d" % (2 * dc.CUT + 1)]
    sizes = [0, 1, dc.CUT, 2 * dc.CUT + 1, 5, 0, 0, dc.CUT + 1]
    return [CASES["random_65280"] if n == dc.CUT else sam[:n] for n in sizes]


def _borders_met(counts, per_slice):
    """From the files' member counts: (a file's last member ends a slice, a file's last member starts a slice, a file
    lies over a slice border, an empty file follows a slice's last member), with more slices behind in every case"""
    total, first = sum(counts), np.concatenate([[0], np.cumsum(counts)])
    spans = [(int(first[f]), int(first[f + 1])) for f in range(len(counts))]
    return (any(a < b < total and b % per_slice == 0 for a, b in spans),
            any(a < b and (b - 1) % per_slice == 0 for a, b in spans),
            any(k % per_slice == 0 for a, b in spans for k in range(a + 1, b)),
            any(0 < a == b < total and a % per_slice == 0 for a, b in spans))


@pytest.fixture(scope="module")
def border_host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("border_host")
    return [dc.host_encode(d, tmp, "f%d" % k) for k, d in enumerate(_border_inputs())]


@pytest.fixture(scope="module")
def border_unset():
    files = variant.bgzf_deflate_many(_border_inputs())
    return files, variant.vcf_stats()


@pytest.mark.parametrize("per_slice", ["1", "2", "3", "0", "99999"])
def test_slice_borders_of_the_vcf_driver(border_host, border_unset, monkeypatch, per_slice):
    inputs = _border_inputs()
    counts = [-(-len(d) // dc.CUT) for d in inputs]
    assert sum(counts) == 8
    if per_slice in ("1", "2", "3"):
        assert _borders_met(counts, int(per_slice)) == (True, True, True, True)
    monkeypatch.setenv("SECEDO_BGZF_SLICE_MEMBERS", per_slice)  # 0 and a value above the writer's 16384: one slice
    files = variant.bgzf_deflate_many(inputs)
    st = variant.vcf_stats()
    assert files == border_host  # every file is the host encoder's
    assert files == border_unset[0]
    for raw, data in zip(files, inputs):
        dc.check_file(raw, data, with_tokens=False)
    assert (st["blocks"], st["stored_blocks"], st["compressed_bytes"]) == (8, 1, sum(map(len, files)))
    for key in ("files", "text_bytes", "blocks", "stored_blocks", "compressed_bytes"):
        assert st[key] == border_unset[1][key], key


@pytest.mark.parametrize("which", ["vcf", "sam"])
def test_ratio_against_zlib_level_1(which):
    """Compressed size over zlib's at level 1 on the same blocks (the bound and the measured quotient are in
    tests/bgzf_deflate_cases.py); no block of compressible text is stored; no member exceeds 64 KiB."""
    data = dc.vcf_like_text() if which == "vcf" else dc.gw.sam_like_text(4000)
    bound = dc.RATIO_VCF_BOUND if which == "vcf" else dc.RATIO_SAM_BOUND
    raw = secedo_amd.bgzf_deflate(data)
    members = dc.check_file(raw, data, with_tokens=False)
    assert variant.vcf_stats()["stored_blocks"] == 0
    assert all(((m[1][0] >> 1) & 3) == 1 for m in members)  # BTYPE 1 everywhere
    ours, (z1, z6) = dc.payload_bytes(raw), dc.zlib_sizes(data)
    print("%s: %d bytes of text, ours %d, zlib level 1 %d, level 6 %d, ours / level 1 = %.4f"
          % (which, len(data), ours, z1, z6, ours / z1))
    assert ours <= bound * z1

"""The DEFLATE encoder of secedo_amd/csrc/bgzf_deflate.hpp on the host: the code the GPU kernel runs, built with g++
under AddressSanitizer and UBSan (secedo_amd/csrc/build/bgzf_deflate_test, which also inflates every member it makes
with the host build of bgzf_inflate.hpp). zlib reads every file back; the headers, BSIZE, CRC32, ISIZE, the cut and the
EOF member are checked field by field."""
import pytest

from tests import bgzf_deflate_cases as dc

CASES = dc.cases()


@pytest.fixture(scope="module")
def encoded(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deflate")
    return {name: dc.host_encode(data, tmp, name) for name, data in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_is_what_bgzip_would_accept(encoded, name):
    dc.check_file(encoded[name], CASES[name])


def test_two_runs_give_the_same_bytes(encoded, tmp_path):
    for name in ("sam_%d" % (2 * dc.CUT + 1), "random_65280", "phrase_at_32768", "empty"):
        assert dc.host_encode(CASES[name], tmp_path, "again") == encoded[name], name


def test_empty_is_the_eof_member_alone(encoded):
    assert encoded["empty"] == dc.gw.EOF_MEMBER


def test_runs_take_distance_one_at_full_length(encoded):
    """A run of n equal bytes: one literal, then matches at distance 1, each as long as a match may be; a rest of
    fewer than 3 bytes (n = 260) is literals."""
    want = {258: [257], 259: [258], 260: [258], 600: [258, 258, 83]}
    for n, lengths in want.items():
        (member, payload, _, _), = dc.split_members(encoded["run_%d" % n])[:-1]
        assert dc.tokens(payload) == [(l, 1) for l in lengths], n


def test_distance_32768_is_taken_and_32769_is_not(encoded):
    (_, payload, _, _), = dc.split_members(encoded["phrase_at_32768"])[:-1]
    assert (40, 32768) in dc.tokens(payload)
    (_, payload, _, _), = dc.split_members(encoded["phrase_at_32769"])[:-1]
    assert all(d <= 258 for _, d in dc.tokens(payload))  # the zeros' own matches only


def test_all_byte_values_are_literals(encoded):
    (_, payload, _, _), = dc.split_members(encoded["all_bytes"])[:-1]
    assert dc.tokens(payload) == [(256, 256)]  # the second copy is one match; the first is 256 literals
    assert len(payload) == (3 + 144 * 8 + 112 * 9 + (7 + 5 + 5 + 6) + 7 + 7) // 8


def test_random_bytes_fall_back_to_a_stored_block(encoded):
    (member, payload, _, isize), = dc.split_members(encoded["random_65280"])[:-1]
    assert payload[0] == 1 and payload[1:5] == bytes([0x00, 0xFF, 0xFF, 0x00])  # BFINAL, BTYPE 0, LEN, NLEN
    assert payload[5:] == CASES["random_65280"] and len(member) == 18 + 5 + 65280 + 8 <= 65536


def test_bit_flush_on_and_off_a_byte_boundary(encoded):
    (_, payload, _, _), = dc.split_members(encoded["flush_aligned"])[:-1]
    assert len(payload) == 8 and dc.tokens(payload) == []  # 64 bits exactly
    (_, payload, _, _), = dc.split_members(encoded["flush_unaligned"])[:-1]
    assert len(payload) == 9 and dc.tokens(payload) == []  # 66 bits


def test_a_match_never_crosses_the_cut(encoded):
    """Each member of the three-member file decodes on its own (check_file) and the first two are full."""
    members = dc.split_members(encoded["sam_%d" % (2 * dc.CUT + 1)])[:-1]
    assert [m[3] for m in members] == [dc.CUT, dc.CUT, 1]
    members = dc.split_members(encoded["sam_%d" % (dc.CUT + 1)])[:-1]
    assert [m[3] for m in members] == [dc.CUT, 1]


@pytest.mark.parametrize("which", ["vcf", "sam"])
def test_ratio_against_zlib_level_1(tmp_path, which):
    """Compressed size over zlib's at level 1 on the same blocks; no block of compressible text is stored."""
    data = dc.vcf_like_text() if which == "vcf" else dc.gw.sam_like_text(4000)
    bound = dc.RATIO_VCF_BOUND if which == "vcf" else dc.RATIO_SAM_BOUND
    raw = dc.host_encode(data, tmp_path, which)
    members = dc.check_file(raw, data, with_tokens=False)
    assert all(((m[1][0] >> 1) & 3) == 1 for m in members)  # BTYPE 1 everywhere
    ours, (z1, z6) = dc.payload_bytes(raw), dc.zlib_sizes(data)
    print("%s: %d bytes of text, ours %d, zlib level 1 %d, level 6 %d, ours / level 1 = %.4f"
          % (which, len(data), ours, z1, z6, ours / z1))
    assert ours <= bound * z1

"""CPU side of the haplotype-resolved `pileup` (-H): the Python BAM reader decodes the HP tag, the record types carry it as a
trailing optional field, and adding that field leaves the synthetic generators' data unchanged."""
import dataclasses
import hashlib
import struct

import numpy as np

from bamutil import aux_B, aux_i, aux_Z, record, write_bgzf

_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}


def _hp(t, v):
    return b"HP" + t.encode() + struct.pack("<" + _FMT[t], v)


def test_aux_tags_decode_integer_hp():
    from hifimeth_amd.bamio import _aux_tags
    mm = aux_Z("MM", "C+m?,0;") + aux_B("ML", np.array([200], np.uint8))
    for t in _FMT:
        for v in (1, 2, 3):
            tags = _aux_tags(aux_Z("RG", "x") + _hp(t, v) + mm)
            assert tags[b"HP"] == v and type(tags[b"HP"]) is int, (t, v)
            assert tags[b"MM"] == "C+m?,0;" and list(tags[b"ML"]) == [200]
    assert _aux_tags(_hp("c", -1))[b"HP"] == -1
    assert _aux_tags(_hp("S", 65535))[b"HP"] == 65535
    assert _aux_tags(_hp("I", 2 ** 32 - 1))[b"HP"] == 2 ** 32 - 1
    assert _aux_tags(aux_Z("HP", "1") + mm).get(b"HP") is None                 # not an integer type
    assert _aux_tags(mm).get(b"HP") is None                                    # no tag
    assert _aux_tags(_hp("C", 2) + _hp("i", 1))[b"HP"] == 2                    # the first of two
    assert _aux_tags(aux_Z("HP", "2") + _hp("i", 1)).get(b"HP") is None        # the first decides, even if not an integer
    assert _aux_tags(aux_B("HP", np.array([1], np.uint8)) + _hp("i", 1)).get(b"HP") is None
    assert _aux_tags(mm, want=(b"MM", b"ML")).get(b"HP") is None


def test_read_bam_carries_hp(tmp_path):
    from hifimeth_amd.bamio import read_bam
    seq4 = np.array([0x12, 0x48], np.uint8)
    auxes = [_hp("c", 1), _hp("I", 2), aux_Z("HP", "1"), b"", _hp("s", 2) + _hp("i", 1), aux_i("XX", 5) + _hp("S", 3)]
    text = "@HD\tVN:1.6\tSO:coordinate\n"
    payload = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", 0)
    payload += b"".join(record(f"r{i}", 4, seq4, 4, aux_Z("MM", "C+m,0;") + a) for i, a in enumerate(auxes))
    path = str(tmp_path / "hp.bam")
    write_bgzf(path, payload)
    recs = list(read_bam(path)[2])
    assert [r.hp for r in recs] == [1, 2, None, None, 2, 3]
    assert all(r.mm == "C+m,0;" for r in recs)


def test_hp_fields_default_to_none():
    from hifimeth_amd.bamio import MappedRecord
    from hifimeth_amd.synth import AlignedRead
    for cls in (MappedRecord, AlignedRead):
        f = dataclasses.fields(cls)[-1]
        assert f.name == "hp" and f.default is None
    a = AlignedRead("a", 0, 0, 0, 60, [("M", 4)], "ACGT", None, None)
    assert a.hp is None and dataclasses.replace(a, hp=2).hp == 2
    m = MappedRecord("m", 0, 0, 0, 60, np.zeros(0, np.uint32), np.zeros(2, np.uint8), 4, None, None)
    assert m.hp is None


def test_synth_alignments_unchanged():
    """the generators' random streams are what they were before the field existed (digest taken from that tree)"""
    from hifimeth_amd.synth import synth_alignments, synth_genome
    g = synth_genome(n_chr=2, length=8000, seed=11)
    h = hashlib.sha256()
    reads = synth_alignments(g, 30, seed=12, median_len=1200)
    for r in reads:
        h.update(repr((r.name, r.flag, r.tid, r.pos, r.mapq, r.cigar, r.seq, r.mm)).encode())
        h.update(b"-" if r.ml is None else bytes(r.ml))
        assert r.hp is None
    assert h.hexdigest() == "97e038e87e066152d51c7f3404b541937456e65bce40d6f04b77a0e7c156d06c"

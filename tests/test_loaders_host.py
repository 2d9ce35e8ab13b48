"""The loader's host-side helpers (annotatedvdb_amd/loaders.py) without an engine:
the batch-then-isolate primary keys, the .mapping text, the capped chromosome
code and the per-alt record descriptor."""

import dataclasses

import pytest

from annotatedvdb_amd import loaders
from annotatedvdb_amd.chromosomes import bin_index_chrom_code
from annotatedvdb_amd.loaders import VCFVariantLoader, _AltRecord, _chrom_code, _mapping_text


class StubPKGenerator:
    """generate_primary_keys refuses the whole call if any metaseq id holds '<'."""

    def __init__(self):
        self.calls = []

    def generate_primary_keys(self, items):
        self.calls.append(list(items))
        for m, _ in items:
            if "<" in m:
                raise ValueError("boom " + m)
        return [m + ":" + ext for m, ext in items]


@pytest.fixture()
def loader():
    ld = VCFVariantLoader.__new__(VCFVariantLoader)  # no engine, no buffers: only the PK generator
    ld._pk_generator = StubPKGenerator()
    return ld


def test_primary_keys_isolates_the_failing_items(loader):
    ok1, bad1, ok2, bad2 = ("1:5:A:C", "rs1"), ("1:6:A:<DEL>", "rs2"), ("2:7:G:T", "rs3"), ("3:8:C:<DUP>", "rs4")
    items = [ok1, bad1, ok2, bad2]
    got = loader._primary_keys(items)
    assert got[0] == "1:5:A:C:rs1" and got[2] == "2:7:G:T:rs3"
    assert [type(g) for g in got] == [str, ValueError, str, ValueError]
    assert str(got[1]) == "boom 1:6:A:<DEL>" and str(got[3]) == "boom 3:8:C:<DUP>"
    assert loader._pk_generator.calls == [items, [ok1], [bad1], [ok2], [bad2]]


def test_primary_keys_one_call_when_all_are_built(loader):
    items = [("1:5:A:C", "rs1"), ("2:7:G:T", "rs3"), ("X:9:T:TA", "rs5")]
    assert loader._primary_keys(items) == ["1:5:A:C:rs1", "2:7:G:T:rs3", "X:9:T:TA:rs5"]
    assert loader._pk_generator.calls == [items]
    assert loader._primary_keys([]) == []


def test_primary_keys_lets_other_exceptions_through(loader):
    with pytest.raises(TypeError):  # ext None: the stub's str + None, no ValueError
        loader._primary_keys([("1:5:A:C", None)])
    assert len(loader._pk_generator.calls) == 1


def test_chrom_code_is_the_capped_bin_index_code():
    loaders._CHROM_CODES.clear()
    labels = ["1", "chr1", "M", "MT", "22", "X", "chrY", "chrUn_KI270302v1", "", "23"]
    for _ in range(2):  # computed, then from the cache
        for x in labels:
            assert _chrom_code(x) == min(bin_index_chrom_code(x), 255), x
    assert _chrom_code("chrUn_KI270302v1") == 255 and _chrom_code("MT") == 255
    assert _chrom_code("1") == _chrom_code("chr1") == 0 and _chrom_code("M") == 24
    assert _chrom_code(1) == 0 and _chrom_code(True) == 255  # keyed by the label's text, not its hash


def test_mapping_text_is_the_drivers_line():
    res = {"1:10177:A:AC": [{"primary_key": "1:10177:A:AC:rs367896724", "bin_index": "chr1.L1.B1"}]}
    assert _mapping_text(res) == "1:10177:A:AC\t" + str(res["1:10177:A:AC"]) + "\n"
    assert _mapping_text(res) == "1:10177:A:AC\t[{'primary_key': '1:10177:A:AC:rs367896724', " \
                                 "'bin_index': 'chr1.L1.B1'}]\n"
    assert _mapping_text({}) == ""
    assert _mapping_text({"a": [], "b": []}) == "a\t[]\nb\t[]\n"


def test_alt_record_fields():
    assert [f.name for f in dataclasses.fields(_AltRecord)] == ["line", "alt", "metaseq", "pk_error", "variant"]
    v = object()
    r = _AltRecord(3, "T", "1:5:A:T", None, v)
    assert (r.line, r.alt, r.metaseq, r.pk_error, r.variant) == (3, "T", "1:5:A:T", None, v)
    err = ValueError("x")
    r.pk_error = err  # set once the key is known to fail
    assert r.pk_error is err
    with pytest.raises(AttributeError):
        r.long = True  # no such slot any more

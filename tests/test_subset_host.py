"""CPU tests of analysis.SubsetWrite and analysis.read_subset: the pinfo tables against a direct restatement of pinfo.c, the header
of write_fileheader (io.c:352-404) as subsetWriteBinaryCharmm fills it (subsetWrite.c:418-484) parsed back, and a written file."""
import numpy as np
import pytest

from ddcmd_amd import analysis
from ddcmd_amd.deck import units_convert

GROUPS = ["free", "bath", "free", "wall", "bath"]                       # indices 2 and 4 repeat a name
SPECIES = ["POPCxNC3", "POPCxPO4", "WxW", "POPCxNC3", "CHOLxROH"]        # index 3 repeats one
TYPES = ["ATOM", "ATOM", "ION", "ATOM", "ION"]
H = [120.0, 0, 0, 0, 90.0, 0, 0, 0, 150.0]


def pinfo_c(groups, species, types):
    """pinfoEncodeInit and pinfoEncode (pinfo.c:15-75, 119-126) restated: maps as the C fills them -- a repeated name is skipped and
    its map entry never written; this restatement gives it the first occurrence's, the object a lookup by that name finds"""
    def codec(names):
        out, m = [], {}
        for i, n in enumerate(names):
            if n in out:
                m[i] = out.index(n)
                continue
            out.append(n)
            m[i] = len(out) - 1
        return out, m
    g_names, g_map = codec(groups)
    s_names, s_map = codec(species)
    t_names, t_map = codec(types)

    def encode(g, s):
        i, j, k = g_map[g], s_map[s], t_map[s]      # itype of a species: the index of its type
        return i + (j + k) * len(g_names) + k * len(s_names)
    return g_names, s_names, t_names, encode


def test_pinfo_tables_against_pinfo_c():
    sw = analysis.SubsetWrite(GROUPS, SPECIES, TYPES)
    g_names, s_names, t_names, encode = pinfo_c(GROUPS, SPECIES, TYPES)
    assert (sw.groups, sw.species_list, sw.types) == (g_names, s_names, t_names) == (["free", "bath", "wall"], ["POPCxNC3", "POPCxPO4", "WxW", "CHOLxROH"], ["ATOM", "ION"])
    assert sw.group_term.dtype == sw.species_term.dtype == np.uint32
    for g in range(len(GROUPS)):
        for s in range(len(SPECIES)):
            assert int(sw.group_term[g]) + int(sw.species_term[s]) == encode(g, s), (g, s)
    assert sw.pinfo_bytes == 1


def test_pinfo_of_a_martini_system_is_group_plus_species_times_groups():
    sw = analysis.SubsetWrite(["group", "free"], ["A", "B", "C"])
    assert list(sw.group_term) == [0, 1] and list(sw.species_term) == [0, 2, 4] and sw.types == ["ATOM"]
    assert list(analysis.SubsetWrite([], ["A"]).group_term) == [0]      # a system without groups: the one group


def test_pinfo_range_beyond_four_bytes_is_refused():
    assert analysis.pinfo_field_size(1, 1, 1) == 1 and analysis.pinfo_field_size(16, 16, 1) == 2
    assert analysis.pinfo_field_size(65536, 65535, 1) == 4
    with pytest.raises(ValueError, match="more than 4"):
        analysis.pinfo_field_size(65536, 65536, 1)
    with pytest.raises(ValueError, match="more than 4"):
        analysis.pinfo_field_size(32, 2 ** 27, 1)


def test_refusals():
    with pytest.raises(ValueError, match="modulus = 0"):
        analysis.SubsetWrite(["g"], ["A"], modulus=0)
    with pytest.raises(ValueError, match="species Z is not a species"):
        analysis.SubsetWrite(["g"], ["A"], species=["A", "Z"])


def _records(n, seed=3):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, analysis.SUBSET_RECORD)
    rec["id"] = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * 2 + 1
    rec["pinfo"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rec["r"] = rng.standard_normal((n, 3)).astype(np.float32) * 40
    return rec


def test_header_parsed_back(tmp_path):
    sw = analysis.SubsetWrite(GROUPS, SPECIES, TYPES, filename="po4", length_unit="nm", modulus=10, odd=1, idmin=3, idmax=99999, species=["WxW"],
                              rmin=[-1.0, -2.0, -3.0], rmax=[1.5, 2.5, 3.5], vmin=[-0.1, -0.2, -0.3], vmax=[0.1, 0.2, 0.3], outputrate=100, h=H)
    assert analysis.SUBSET_RECORD.itemsize == 24
    rec = _records(7)
    path = sw.write(str(tmp_path), rec, loop=1200, time=units_convert(24000.0, "fs", None), h=H, version="v-test")
    assert path.endswith("po4#000000") and not (tmp_path / "po4#000000.tmp").exists()
    hdr, back = analysis.read_subset(path)
    assert hdr["name"] == "subset" and hdr["type"] == "MULTILINE" and hdr["datatype"] == "FIXRECORDBINARY" and hdr["checksum"] == "NONE"
    assert hdr["code_version"] == "v-test" and hdr["srcpath"] == "libddcmi" and hdr["run_id"] == "0x00000000"
    assert (hdr["nfiles"], hdr["nrecord"], hdr["lrec"], hdr["nfields"], hdr["loop"]) == (1, 7, 24, 5, 1200)
    assert hdr["endian_key"] == int(np.frombuffer(b"1234", "<i4")[0])
    assert hdr["time"] == "24000.000000 fs"
    assert hdr["field_names"] == ["id", "pinfo", "rx", "ry", "rz"] and hdr["field_types"] == ["u8", "u4", "f4", "f4", "f4"]
    assert hdr["field_units"] == ["1", "1", "nm", "nm", "nm"]
    assert hdr["reducedcorner"].split() == ["-0.50000000000000"] * 3
    ang = units_convert(1.0, None, "Angstrom")
    assert hdr["h"] == pytest.approx([x * ang for x in H], abs=1e-13)
    assert hdr["random"] == "NONE" and hdr["nrandomFieldSize"] == "0"
    assert hdr["types"] == ["ATOM", "ION"] and hdr["groups"] == ["free", "bath", "wall"] and hdr["species"] == ["POPCxNC3", "POPCxPO4", "WxW", "CHOLxROH"]
    assert (hdr["idmin"], hdr["idmax"], hdr["modulus"], hdr["odd"]) == ("3", "99999", "10", "1")
    vel = units_convert(1.0, None, "Angstrom/fs")
    assert hdr["xmin"] == "%f Ang" % (-1.0 * ang) and hdr["zmax"] == "%f Ang" % (3.5 * ang) and hdr["vymax"] == "%f Ang/fs" % (0.2 * vel)
    assert back.dtype == analysis.SUBSET_RECORD and back.tobytes() == rec.tobytes()


def test_header_text_line_by_line():
    """write_fileheader's lines in its order, the misc_info block in subsetWriteBinaryCharmm's"""
    sw = analysis.SubsetWrite(["group"], ["WxW"], h=H)
    lines = sw.header(5, 10, 0.0, H, version="x", create_time="T").split("\n")
    assert lines[0] == "subset FILEHEADER {type=MULTILINE; datatype=FIXRECORDBINARY; checksum=NONE; create_time=T; run_id=0x00000000;"
    assert lines[1] == "code_version=x; srcpath=libddcmi;" and lines[2] == "loop=10; time=0.000000 fs;"
    assert lines[3] == "nfiles=1; nrecord=5; lrec=24; nfields=5; endian_key=%d;" % int(np.frombuffer(b"1234", "<i4")[0])
    assert lines[4:7] == ["field_names=id pinfo rx ry  rz;", "field_types= u8 u4 f4 f4 f4;", "field_units=1 1 Ang Ang Ang;"]
    assert lines[7].startswith("reducedcorner=") and lines[8].startswith("h=") and lines[10].endswith(" Ang;")
    assert [ln.strip() for ln in lines[11:17]] == ["random = NONE;", "nrandomFieldSize = 0;", "types = ATOM ;", "groups = group ;", "species = WxW ;",
                                                  "idmin = 0; idmax = 18446744073709551615; modulus = 1; odd = 0;"]
    assert lines[17].startswith("xmin = ") and lines[22].startswith("vzmin = ")
    assert lines[23:] == ["", "}", " ", "", ""]


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_a_written_file_round_trips(tmp_path, n):
    sw = analysis.SubsetWrite(["group"], ["WxW", "WFxWF"], h=H)
    rec = _records(n, seed=n)
    raw = sw.file_bytes(rec, 20, 1.0, H)
    assert len(raw) == len(sw.header(n, 20, 1.0, H)) + 24 * n
    hdr, back = analysis.read_subset(sw.write(str(tmp_path), rec, 20, 1.0, H))
    assert hdr["nrecord"] == n and back.tobytes() == rec.tobytes()
    for k in ("id", "pinfo", "r"):
        assert np.array_equal(back[k], rec[k])


def test_a_truncated_file_is_refused(tmp_path):
    sw = analysis.SubsetWrite(["group"], ["WxW"], h=H)
    path = sw.write(str(tmp_path), _records(4), 20, 1.0, H)
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-5])
    with pytest.raises(ValueError, match="nrecord"):
        analysis.read_subset(path)

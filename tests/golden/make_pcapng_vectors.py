#!/usr/bin/env python3
"""Regenerate tests/golden/pcapng_vectors.json and tests/golden/pcapng/{le,be}/*.pcapng from a
checkout of google/gopacket:

    python tests/golden/make_pcapng_vectors.py /path/to/gopacket

The capture files are pcapgo/tests/{le,be}/*.pcapng, copied as they are (data).  The vectors
are the expectations of pcapgo/ngread_test.go's `tests` table (the table TestNgFileRead{LE,BE}
run over both directories), read from the Go file AS TEXT with the small composite-literal
parser below — nothing of the Go text is kept but names, numbers and strings:

  per test      testName, the three NgReaderOptions flags, linkType
  per section   the NgSectionInfo strings and every interface's LinkType, SnapLength, Name,
                Comment, Description, Filter, OS, TimestampResolution (0 -> 6 as the Go test's
                checkInterface does), TimestampOffset, and its Statistics as written
  per packet    data (hex), Timestamp as Unix seconds + nanoseconds (zero_time for time.Time{}),
                Length, CaptureLength, InterfaceIndex, the AncillaryData link type; or the
                expected error's text

(The helpers of make_golden.py read single literals at an anchor; this table is nested, so it
has a parser of its own; line_of below is the same helper.)
"""
import json
import os
import re
import shutil
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
SRC = "pcapgo/ngread_test.go"

LINKTYPES = {"layers.LinkTypeNull": 0, "layers.LinkTypeEthernet": 1}
ERRORS = {  # pcapgo/pcapng.go:19,22
    "ErrNgVersionMismatch": "Unknown pcapng Version in Section Header",
    "ErrNgLinkTypeMismatch": "Link type of current interface is different from first one",
}
NO_VALUE_64 = (1 << 64) - 1  # NgNoValue64, pcapng.go:121


def line_of(src, anchor):
    return src[:src.index(anchor)].count("\n") + 1


class Lit:
    """A Go composite literal: type text + keyed fields or a list of elements."""

    def __init__(self, typ):
        self.typ, self.fields, self.items = typ, {}, []


def parse_value(s, i):
    """An expression starting at s[i]: a Lit or the expression's text; returns (value, next i)."""
    depth, j, in_str = 0, i, False
    while True:
        c = s[j]
        if in_str:
            if c == "\\":
                j += 1
            elif c == '"':
                in_str = False
        elif c == '"':
            in_str = True
        elif c in "([":
            depth += 1
        elif c in ")]":
            depth -= 1
        elif depth == 0 and c == "{":
            typ = s[i:j].strip()
            if s[j + 1] == "}" and typ.endswith("interface"):  # []interface{}{...}
                typ, j = typ + "{}", j + 2
            return parse_body(s, j + 1, typ)
        elif depth == 0 and c in ",}":
            return s[i:j].strip(), j
        j += 1


def parse_body(s, i, typ):
    lit = Lit(typ)
    while True:
        m = re.compile(r"(\s|//[^\n]*)*").match(s, i)
        i = m.end()
        if s[i] == "}":
            return lit, i + 1
        k = re.compile(r"([A-Za-z_]\w*)\s*:").match(s, i)
        if k:
            v, i = parse_value(s, k.end())
            lit.fields[k.group(1)] = v
        else:
            v, i = parse_value(s, i)
            lit.items.append(v)
        m = re.compile(r"(\s|//[^\n]*)*").match(s, i)
        i = m.end()
        if s[i] == ",":
            i += 1


def go_int(expr):
    if expr == "NgNoValue64":
        return NO_VALUE_64
    if not re.fullmatch(r"[0-9a-fA-Fx+\-* ()]+", expr):
        raise ValueError("not an integer expression: " + expr)
    return eval(expr)  # Go's integer syntax here is Python's: decimal, 0x.., + - *


def go_string(expr):
    return json.loads(expr)  # the table's strings are plain ASCII without escapes


def go_time(v):
    """time.Unix(sec, nsec).UTC() -> normalised (sec, nsec, zero_time)."""
    if isinstance(v, Lit):
        assert v.typ == "time.Time" and not v.fields and not v.items
        return {"zero_time": True, "ts_sec": 0, "ts_nsec": 0}
    m = re.fullmatch(r"time\.Unix\((.*),(.*)\)\.UTC\(\)", v)
    sec, nsec = go_int(m.group(1).strip()), go_int(m.group(2).strip())
    sec, nsec = sec + nsec // 10**9, nsec % 10**9
    return {"zero_time": False, "ts_sec": sec, "ts_nsec": nsec}


def main():
    src = open(os.path.join(REF, SRC)).read()
    sources = [m for m in re.findall(r'ngMustDecode\("([0-9a-f]*)"\)', src)]
    start = src.index("var tests = []ngFileReadTest{")
    table, _ = parse_value(src, start + len("var tests = "))

    def data_of(expr):
        m = re.fullmatch(r"ngPacketSource\[(\d+)\](?:\[:(\d+)\])?", expr)
        b = bytes.fromhex(sources[int(m.group(1))])
        return b[:int(m.group(2))] if m.group(2) else b

    def length_of(expr):
        m = re.fullmatch(r"len\(ngPacketSource\[(\d+)\]\)", expr)
        return len(bytes.fromhex(sources[int(m.group(1))])) if m else go_int(expr)

    tests = []
    for t in table.items:
        f = t.fields
        assert "testContents" not in f
        out = {
            "name": go_string(f["testName"]),
            "type": go_string(f.get("testType", '""')),
            "line": line_of(src, "testName: " + f["testName"]) if ("testName: " + f["testName"]) in src
            else line_of(src, f["testName"]),
            "want_mixed_linktype": f.get("wantMixedLinkType") == "true",
            "error_on_mismatching_linktype": f.get("errorOnMismatchingLinkType") == "true",
            "skip_unknown_version": f.get("skipUnknownVersion") == "true",
            "linkType": LINKTYPES[f["linkType"]] if "linkType" in f else 0,
            "sections": [],
            "packets": [],
        }
        for s in f["sections"].items if "sections" in f else []:
            info = s.fields.get("sectionInfo")
            sec = {k: go_string(info.fields.get(k, '""')) if info else ""
                   for k in ("Hardware", "OS", "Application", "Comment")}
            ifaces = []
            for it in s.fields["ifaces"].items if "ifaces" in s.fields else []:
                g = it.fields
                known = {"LinkType", "SnapLength", "Name", "Comment", "Description", "Filter", "OS",
                         "TimestampResolution", "TimestampOffset", "Statistics"}
                assert set(g) <= known, set(g) - known
                d = {k: go_string(g.get(k, '""')) for k in ("Name", "Comment", "Description", "Filter", "OS")}
                d["LinkType"] = LINKTYPES[g["LinkType"]] if "LinkType" in g else 0
                d["SnapLength"] = go_int(g.get("SnapLength", "0"))
                d["TimestampResolution"] = go_int(g.get("TimestampResolution", "0")) or 6
                d["TimestampOffset"] = go_int(g.get("TimestampOffset", "0"))
                if "Statistics" in g:
                    st = g["Statistics"].fields
                    d["Statistics"] = {k: (go_time(v) if k in ("LastUpdate", "StartTime", "EndTime")
                                           else go_string(v) if k == "Comment" else go_int(v))
                                       for k, v in st.items()}
                ifaces.append(d)
            out["sections"].append({"sectionInfo": sec, "ifaces": ifaces})
        for p in f["packets"].items if "packets" in f else []:
            g = p.fields
            if "err" in g:
                out["packets"].append({"err": ERRORS[g["err"]]})
                continue
            ci = g["ci"].fields
            assert set(ci) <= {"Timestamp", "Length", "CaptureLength", "InterfaceIndex", "AncillaryData"}, set(ci)
            d = {"data": data_of(g["data"]).hex()}
            d.update(go_time(ci["Timestamp"]))
            d["Length"] = length_of(ci["Length"])
            d["CaptureLength"] = length_of(ci["CaptureLength"])
            d["InterfaceIndex"] = go_int(ci.get("InterfaceIndex", "0"))
            if "AncillaryData" in ci:
                (lt,) = ci["AncillaryData"].items
                d["linktype"] = LINKTYPES[lt]
            out["packets"].append(d)
        tests.append(out)

    files = {}
    for e in ("le", "be"):
        dst = os.path.join(OUT, "pcapng", e)
        os.makedirs(dst, exist_ok=True)
        names = sorted(n for n in os.listdir(os.path.join(REF, "pcapgo", "tests", e)) if n.endswith(".pcapng"))
        for n in names:
            shutil.copyfile(os.path.join(REF, "pcapgo", "tests", e, n), os.path.join(dst, n))
        files[e] = names
    doc = {
        "source": SRC,
        "table_line": line_of(src, "var tests = []ngFileReadTest{"),
        "note": "TimestampResolution 0 is recorded as 6 (checkInterface, ngread_test.go:85-88). "
                "Statistics are recorded as written in the table; the native reader parses "
                "statistics blocks and drops their values, so the tests do not compare them.",
        "omitted": [],
        "not_compared": ["Statistics"],
        "files": files,
        "tests": tests,
    }
    with open(os.path.join(OUT, "pcapng_vectors.json"), "w") as fo:
        json.dump(doc, fo, indent=1, sort_keys=True)
        fo.write("\n")
    print("%d tests, %d packets, %d files" % (len(tests), sum(len(t["packets"]) for t in tests),
                                              sum(len(v) for v in files.values())))


if __name__ == "__main__":
    main()

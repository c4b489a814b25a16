"""Writes tests/golden/hand_text.sam and hand_text_records.json from one table of field values: the SAM lines, and the BAM
records they must become, spelled field by field with struct (SAM/BAM specification 4.2).  Nothing
here imports the model or the library.

    python tests/golden/make_hand_text_sam.py
"""
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
REFS = [("chr1", 1000), ("chr2", 2000), ("chrM", 16569)]
HEADER = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in REFS) + "@CO\thand-worked records for SAM to BAM\n"
OPS = "MIDNSHP=X"
NIB = "=ACMGRSVTWYHKDBN"


def fixed(ref, pos, l_rn, mapq, bin_, n_op, flag, l_seq, nref, npos, tlen):
    return struct.pack("<iiBBHHHIiii", ref, pos, l_rn, mapq, bin_, n_op, flag, l_seq, nref, npos, tlen)


def cig(*ops):
    return b"".join(struct.pack("<I", n << 4 | OPS.index(o)) for n, o in ops)


def seq(s):
    n = [NIB.index(c) for c in s.upper()] + [0]
    return bytes(n[k] << 4 | n[k + 1] for k in range(0, len(s), 2))


def rec(body):
    return struct.pack("<I", len(body)) + body


# (line, record): the line's fields are the table; the record is spelled beside it
TABLE = []

# every CIGAR operation, odd l_seq, RNEXT "=", an A tag and the six integer widths at their boundaries
TABLE.append((
    ["r0", "99", "chr1", "11", "60", "2S3M1I1D2N1P2=1X1H", "=", "51", "100", "ACGTN", "IIII!",
     "XA:A:q", "a0:i:0", "a1:i:255", "a2:i:256", "a3:i:65535", "a4:i:65536", "a5:i:4294967295", "a6:i:-1", "a7:i:-128", "a8:i:-129",
     "a9:i:-32768", "aa:i:-32769", "ab:i:-2147483648"],
    # span = 3M + 1D + 2N + 2= + 1X = 9; pos 10..19 lies in one 16 kb window: bin 4681
    rec(fixed(0, 10, 3, 60, 4681, 9, 99, 5, 0, 50, 100) + b"r0\0" +
        cig((2, "S"), (3, "M"), (1, "I"), (1, "D"), (2, "N"), (1, "P"), (2, "="), (1, "X"), (1, "H")) + seq("ACGTN") + bytes([40, 40, 40, 40, 0]) +
        b"XAAq" + b"a0C" + struct.pack("<B", 0) + b"a1C" + struct.pack("<B", 255) + b"a2S" + struct.pack("<H", 256) + b"a3S" + struct.pack("<H", 65535) +
        b"a4I" + struct.pack("<I", 65536) + b"a5I" + struct.pack("<I", 4294967295) + b"a6c" + struct.pack("<b", -1) + b"a7c" + struct.pack("<b", -128) +
        b"a8s" + struct.pack("<h", -129) + b"a9s" + struct.pack("<h", -32768) + b"aai" + struct.pack("<i", -32769) + b"abi" + struct.pack("<i", -2147483648))))

# even l_seq in lower case, absent qualities, RNEXT another name, Z H f
TABLE.append((
    ["r1", "147", "chr2", "1500", "0", "8M", "chrM", "16000", "-300", "acgtmrsv", "*",
     "ZZ:Z:hello world", "ZE:Z:", "HH:H:1AE301", "ff:f:1.5", "fn:f:-0.1", "fi:f:inf", "fe:f:1e-45"],
    rec(fixed(1, 1499, 3, 0, 4681, 1, 147, 8, 2, 15999, -300) + b"r1\0" + cig((8, "M")) + seq("ACGTMRSV") + b"\xff" * 8 +
        b"ZZZhello world\0" + b"ZEZ\0" + b"HHH1AE301\0" + b"fff" + struct.pack("<f", 1.5) + b"fnf" + struct.pack("<I", 0xBDCCCCCD) +
        b"fif" + struct.pack("<I", 0x7F800000) + b"fef" + struct.pack("<I", 1))))

# an unplaced record without CIGAR, SEQ and QUAL; all seven B subtypes and an empty array
TABLE.append((
    ["unplaced", "4", "*", "0", "0", "*", "*", "0", "0", "*", "*",
     "b0:B:c,-128,127", "b1:B:C,0,255", "b2:B:s,-32768,32767", "b3:B:S,0,65535", "b4:B:i,-2147483648,2147483647", "b5:B:I,0,4294967295",
     "b6:B:f,0.5,1000000000,-0", "b7:B:c"],
    rec(fixed(-1, -1, 9, 0, 4680, 0, 4, 0, -1, -1, 0) + b"unplaced\0" +
        b"b0Bc" + struct.pack("<Ibb", 2, -128, 127) + b"b1BC" + struct.pack("<IBB", 2, 0, 255) + b"b2Bs" + struct.pack("<Ihh", 2, -32768, 32767) +
        b"b3BS" + struct.pack("<IHH", 2, 0, 65535) + b"b4Bi" + struct.pack("<Iii", 2, -2147483648, 2147483647) +
        b"b5BI" + struct.pack("<III", 2, 0, 4294967295) + b"b6Bf" + struct.pack("<I", 3) + struct.pack("<ff", 0.5, 1e9) + struct.pack("<I", 0x80000000) +
        b"b7Bc" + struct.pack("<I", 0))))

# every SEQ letter, RNEXT "*" beside a placed RNAME, QNAME "*", a span that crosses a 16 kb window (bin of the 128 kb level)
TABLE.append((
    ["*", "16", "chrM", "16380", "255", "16M", "*", "0", "0", "=ACMGRSVTWYHKDBN", "!\"#$%&'()*+,-./~"],
    # pos 16379, end 16395: 16379 >> 14 = 0, 16394 >> 14 = 1; >> 17 both 0: bin 585
    rec(fixed(2, 16379, 2, 255, 585, 1, 16, 16, -1, -1, 0) + b"*\0" + cig((16, "M")) + bytes([0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF]) +
        bytes(list(range(0, 15)) + [93]))))

if __name__ == "__main__":
    with open(os.path.join(HERE, "hand_text.sam"), "w", newline="") as f:
        f.write(HEADER + "".join("\t".join(fields) + "\n" for fields, _ in TABLE))
    with open(os.path.join(HERE, "hand_text_records.json"), "w") as f:
        json.dump({"header_text": HEADER, "references": REFS, "records": [r.hex() for _, r in TABLE]}, f, indent=1)
        f.write("\n")

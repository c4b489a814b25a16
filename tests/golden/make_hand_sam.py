#!/usr/bin/env python3
"""hand_spec.sam: the SAM text of hand_spec.bam, worked out by hand from the RECORDS table of make_hand_bam.py with the rules
of DESIGN.md section 13.1 -- NOT with tests/sam_model.py, which test_convert.py holds to this file.  Only the long runs are
spelled by Python below (the filler strings, repeated bases, runs of one quality); every field is written as text.

    python tests/golden/make_hand_sam.py        (re-creates hand_spec.sam)
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
filler = " ".join("token%04d:%s" % (k, "ACGT"[k % 4] * (k % 7 + 1)) for k in range(160))   # as make_hand_bam.py

HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:5000\n@CO\thand-assembled from the specification\n"
LINES = [
    # r1: POS 99 -> 100, the mate on its own sequence -> "=", PNEXT 300 -> 301; QUAL 30..40 cycling by 11 -> "?".."I";
    # every tag type: c C s S i I all as "i", 3.5 as "3.5", the Z value keeps its tab, 1e10 as an f32 is 10000000000 exactly,
    # the empty B:C array is "B:C"
    "\t".join(["r1/all_tags", "99", "chr1", "100", "60", "50M", "=", "301", "251", "ACGTN" * 10,
               "".join("?@ABCDEFGHI"[i % 11] for i in range(50)),
               "XA:A:Q", "Xc:i:-7", "XC:i:250", "Xs:i:-30000", "XS:i:60000", "Xi:i:-2000000000", "XI:i:4000000000", "Xf:f:3.5",
               "XZ:Z:a string with spaces \t and a tab", "XH:H:1AE301", "Bc:B:c,-1,2,-3", "BC:B:C,1,2,255", "Bs:B:s,-300,300",
               "BS:B:S,65535", "Bi:B:i,-70000,70000", "BI:B:I,1,4000000000", "Bf:B:f,0.25,-1.5,10000000000", "BZ:B:C",
               "ZZ:Z:" + filler]),
    # r2: 20 x Q2 -> "#", 30 x Q40 -> "I"
    "\t".join(["r2", "147", "chr1", "301", "60", "20S30M", "=", "100", "-251", "G" * 20 + "ACGT" * 7 + "AC", "#" * 20 + "I" * 30,
               "NM:i:1", "YY:Z:" + filler[::-1]]),
    # r3: no mate (RNEXT *, PNEXT 0), qualities 0xFF -> "*"
    "\t".join(["r3", "0", "chr1", "321", "0", "10M2I5M3D10M100N5M1X4=", "*", "0", "0",
               "ACGTACGTAC" + "TT" + "GGGGG" + "ACGTACGTAC" + "CCCCC" + "A" + "TTTT", "*", "XX:Z:" + filler * 2]),
    # r4: MAPQ 255 stays 255, Q93 -> "~", no tags
    "\t".join(["r4", "1040", "chr1", "5001", "255", "5H40M5H", "*", "0", "0", "ACGT" * 10, "~" * 40]),
    # r5: all 16 base codes, Q0 -> "!"
    "\t".join(["r5", "256", "chr1", "5011", "3", "40M", "*", "0", "0", "=ACMGRSVTWYHKDBN" * 2 + "ACGTACGT", "!" * 40]),
    # r6: the mate on another sequence -> its name; Q10..19 -> "+" .. "4"
    "\t".join(["r6/straddles", "65", "chr1", "99991", "20", "10M", "chr2", "11", "0", "AAAAACCCCC", "+,-./01234", "RG:Z:group"]),
    # r7: Q20 -> "5"
    "\t".join(["r7", "129", "chr2", "11", "20", "120M", "chr1", "99991", "0", "ACGT" * 30, "5" * 120]),
    # r8: unplaced: RNAME *, POS 0, CIGAR *; Q5 -> "&"
    "\t".join(["r8/unplaced", "77", "*", "0", "0", "*", "*", "0", "0", "N" * 10, "&" * 10]),
]
with open(os.path.join(HERE, "hand_spec.sam"), "wb") as f:
    f.write((HEADER + "".join(line + "\n" for line in LINES)).encode())
print("hand_spec.sam", len(LINES), "records")

"""Copies the data files the reference's alignment-properties unit tests read (src/estimation/alignment_properties.rs:1057-1120)
into tests/golden/alignment_properties/, byte for byte, from a checkout of the reference given as the only argument:

    python tools/make_alignment_properties_fixtures.py PATH/TO/varlociraptor

tumor-first30000.bam (3.7 MB, the input of `test_estimate`) is larger than the 1 MiB limit of a committed file and is not copied
(its pinned numbers are not checked by the suite).
"""
import os
import shutil
import sys

FILES = ("tumor-first30000.reads_with_soft_clips.bam", "tumor-first30000.reads_with_soft_clips.bam.bai",
         "tumor-first30000.reads_with_soft_clips.bam.csi", "tumor-first30000.bunch_of_reads_made_single_ended.bam",
         "tumor-first30000.bunch_of_reads_made_single_ended.bam.csi", "chr10.fa", "chr10.fa.fai")
DST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "alignment_properties")

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(sys.argv[1], "tests", "resources")
    os.makedirs(DST, exist_ok=True)
    for f in FILES:
        shutil.copyfile(os.path.join(src, f), os.path.join(DST, f))
        print(f, os.path.getsize(os.path.join(DST, f)))

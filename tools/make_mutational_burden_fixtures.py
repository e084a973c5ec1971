"""Copies the data file of the reference's mutational-burden test case (tests/resources/testcases/test_tmb/annotated.vcf: 39 SNV
records with SnpEff ANN annotations, samples `normal` and `tumor`) into tests/golden/mutational_burden/, byte for byte, from a
checkout of the reference given as the only argument:

    python tools/make_mutational_burden_fixtures.py PATH/TO/varlociraptor
"""
import os
import shutil
import sys

FILES = ("annotated.vcf",)
DST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mutational_burden")

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(sys.argv[1], "tests", "resources", "testcases", "test_tmb")
    os.makedirs(DST, exist_ok=True)
    for f in FILES:
        shutil.copyfile(os.path.join(src, f), os.path.join(DST, f))
        print(f, os.path.getsize(os.path.join(DST, f)))

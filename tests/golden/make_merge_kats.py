#!/usr/bin/env python3
"""Generate tests/golden/merge_kats.json: the two known-answer tests the reference holds for merge_exact (src/merge/strategy/exact.rs,
test_merge_exact and test_merge_exact_phasing).

    python tests/golden/make_merge_kats.py <root of the reference's source tree>

Run ONCE where the reference's sources are.  The fixture is DATA: inputs and expected values pulled out of the reference's test module by
regular expressions, each case tagged with the file:line it was read from; no source text is stored.  Genotype values are written as
["U", i] Unphased(i), ["P", i] Phased(i), ["U", null] UnphasedMissing, ["P", null] PhasedMissing."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = "src/merge/strategy/exact.rs"
GT = r"GenotypeAllele::(Unphased|Phased)(Missing)?(?:\((\d+)\))?"


def gts(text):
    return [[m.group(1)[0], None if m.group(2) else int(m.group(3))] for m in re.finditer(GT, text)]


def main(ref):
    src = open(os.path.join(ref, PATH)).read()
    tests = src[src.index("mod tests"):]
    cases = []
    for m in re.finditer(r"#\[test\]\s*fn (\w+)\(\) \{(.*?)\n    \}", tests, re.S):
        name, body = m.group(1), m.group(2)
        line = src[:src.index("fn " + name + "(")].count("\n") + 1
        gt_text = re.search(r"let sample_gts = vec!\[(.*?)\n        \];", body, re.S).group(1)
        al_text = re.search(r"let sample_alleles = vec!\[(.*?)\n        \];", body, re.S).group(1)
        vcf_gts = [[gts(e.group(1))] for e in re.finditer(r"vec!\[vec!\[(.*?)\]\]", gt_text, re.S)]
        sample_alleles = [re.findall(r'b"([A-Z]+)"', e.group(1)) for e in re.finditer(r"vec!\[(.*?)\n            \]", al_text, re.S)]
        assert len(vcf_gts) == len(sample_alleles) > 0, name
        expect = dict(first=re.search(r'sorted_alleles\[0\],\s*b"([A-Z]+)"', body).group(1),
                      n_alleles=int(re.search(r"sorted_alleles\.len\(\), (\d+)", body).group(1)),
                      out_gts=[[int(e.group(1)), int(e.group(2)), gts(e.group(3))]
                               for e in re.finditer(r"out_gts\[(\d+)\]\[(\d+)\],\s*vec!\[(.*?)\]", body, re.S)])
        assert expect["out_gts"], name
        cases.append(dict(name=name, source="exact.rs:%d" % line, vcf_gts=vcf_gts, sample_alleles=sample_alleles, expect=expect))
    assert [c["name"] for c in cases] == ["test_merge_exact", "test_merge_exact_phasing"], [c["name"] for c in cases]
    with open(os.path.join(HERE, "merge_kats.json"), "w") as f:
        json.dump(dict(reference="PacificBiosciences/trgt v3.0.0, " + PATH, cases=cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])

"""Measures the two recorded bounds of the sample-preparation restatement (tests/sample_ref.py) and writes them under
"restatement_bounds" of profiles/sample_prep.json:  python tools/sample_prep_bounds.py
  warp_noise_max / warp_noise_hist   |fixed-point cubic warp - float64 Keys bicubic at the exact coordinate| on a noise image (17 degrees)
  colour_roundtrip_max               |BGR -> HSV -> BGR - BGR| on the 32^3 lattice, all greys and the saturated primaries
tests/test_samples_host.py measures the same again and asserts the recorded maximum plus one level."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import test_samples_host as T          # noqa: E402
from conftest import pkg               # noqa: E402


def main():
    mx, hist = T.warp_noise_difference(pkg('samples'))
    out = json.load(open(T.BOUNDS)) if os.path.exists(T.BOUNDS) else {}
    out['restatement_bounds'] = dict(warp_noise_max=mx, warp_noise_hist=hist, colour_roundtrip_max=T.colour_roundtrip_max(),
                                     note='hist[k] = pixels with floor(|difference|) = k, interior pixels of a 40 x 52 noise image')
    json.dump(out, open(T.BOUNDS, 'w'), indent=1, sort_keys=True)
    print(json.dumps(out['restatement_bounds']))


if __name__ == '__main__':
    main()

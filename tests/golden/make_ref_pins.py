"""Generates tests/golden/ref_pins.json: the SHA-256 of what the REAL reference (oracle/_ref, built by `make -C oracle ref`)
writes for every case of tests/test_oracle.py's differential tests (random planes, extreme tables, every tier and public
dispatcher, the property-based cases hypothesis draws), so that those tests compare the oracle with the reference without it.

Run where the reference sources exist, on a host with AVX-512VL (every tier must run):
    make -C oracle ref && python tests/golden/make_ref_pins.py
The file holds hashes and case parameters only.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle as O  # noqa: E402
import test_oracle as T  # noqa: E402


def main():
    assert O.reference() is not None, "build oracle/_ref first: make -C oracle ref"
    flags = O.host_cpu_flags()
    pins = {"random": {}, "extreme": {}, "tiers": {}, "public": {}, "property": []}
    for beh in O.REF_FUNCS:
        for W, H, scale, img, lut in T.random_cases():
            for (y0, y1) in T.random_ranges(H):
                _, out = O.run_behaviour(beh, img, lut, W, H, y0, y1, out=np.full(W * H, 0x5A, dtype=np.uint8), use_reference=True)
                pins["random"][T.case_key(beh, f"{W}x{H}", scale, y0, y1)] = T._sha(out)
    for special, img, lut in T.extreme_cases():
        for beh in O.REF_FUNCS:
            _, out = O.run_behaviour(beh, img, lut, 64, 16, 0, 16, out=np.zeros(64 * 16, dtype=np.uint8), use_reference=True)
            pins["extreme"][T.case_key(beh, special)] = T._sha(out)
    tiers = sorted(set(T.TIER_SAME) | {p for p, _ in T.TIER_SAME.values()})
    assert all(O.REF_TIERS[t][1] in flags for t in tiers) and "sse4_1" in flags, "this host cannot run every tier"
    for W, H, scale, img, lut in T.tier_cases():
        for (y0, y1) in T.tier_ranges(H):
            geom = (f"{W}x{H}", scale, y0, y1)
            for t in tiers:
                pins["tiers"][T.case_key(t, *geom)] = T._sha(O.run_tier(t, img, lut, W, H, y0, y1, out=np.full(W * H, 0x5A, dtype=np.uint8)))
            for which, _ in T.TIER_PUBLIC:
                rc, out = O.run_public(which, img, lut, W, H, y0, y1, out=np.full(W * H, 0x5A, dtype=np.uint8))
                assert rc == 0
                pins["public"][T.case_key(which, *geom)] = T._sha(out)

    import hypothesis as hyp
    import hypothesis.strategies as st

    seen = set()

    def record(**case):
        def digest(W, H, img, lut):
            out = np.full(W * H, 0xC3, dtype=np.uint8)
            O.run_behaviour(case["beh"], img, lut, W, H, case["y0"], case["y1"], out=out, use_reference=True)
            sha = T._sha(out)
            key = json.dumps(case, sort_keys=True)
            if key not in seen:
                seen.add(key)
                pins["property"].append(dict(case, sha256=sha))
            return sha
        T.property_check(**case, digest=digest)

    T.property_strategy_check(hyp, st, record)()
    with open(os.path.join(HERE, "ref_pins.json"), "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in pins.items()})


if __name__ == "__main__":
    main()

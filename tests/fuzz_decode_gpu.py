"""The long-run form of tests/test_gpu_decode_cases.py (not part of the default suite beyond a three-second entry; run on the GPU box
from the repo root: python tests/fuzz_decode_gpu.py [seconds] [first_seed]).  Windows of tests/decode_cases.py by ascending seed,
from beyond the committed list by default; per window the beam, the exact path, the max-marginals, the k best and score_paths
against the plain references, the same once more after viterbi_spin(2) on both sides (tests/decode_checks.py, items 1-5 and 7).
It stops at the first mismatch and prints the window's description: there is no retry."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import decode_cases
import decode_checks

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else decode_cases.FUZZ_FIRST_SEED
first = seed
t_end = time.time() + budget
by_s, by_states = {}, {}
n_cases = n_holes = n_beyond = 0
BINS = ((1, "1"), (16, "2..16"), (256, "17..256"), (1024, "257..1024"), (4095, "1025..4095"), (4096, "4096"))
while time.time() < t_end:
    desc, t = decode_cases.case(seed)
    h, o = decode_checks.pair_of(desc, t)
    ref = decode_cases.references(desc, o)
    seed += 1
    if ref["over"]:                                          # (the refusals: item 6, the suite's)
        n_beyond += 1
        continue
    try:
        decode_checks.same_exact(decode_checks.gpu_exact(h, desc["K"]), ref, desc["N"])
        decode_checks.check_beam(h, desc, ref)
        decode_checks.check_score(h, o, desc, ref)
        decode_checks.check_reweighted(h, o, desc)
    except AssertionError as e:
        print("MISMATCH", e, desc, flush=True)
        sys.exit(1)
    except Exception as e:
        print("ERROR", repr(e), desc, flush=True)
        sys.exit(1)
    n_cases += 1
    sh = ref["shape"]
    if ref["vit"]["hole_at"]:
        n_holes += 1
        continue
    by_s[sh["S"]] = by_s.get(sh["S"], 0) + 1
    name = next(label for top, label in BINS if sh["states"] <= top)
    by_states[name] = by_states.get(name, 0) + 1
print("fuzz ok: %d windows from seed %d (%d of them with a hole, %d more beyond the cap), by S %s, by states %s"
      % (n_cases, first, n_holes, n_beyond, dict(sorted(by_s.items())), {label: by_states[label] for _, label in BINS if label in by_states}))

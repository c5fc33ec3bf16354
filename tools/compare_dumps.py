"""Compare two `bench.py --dump-outputs` directories byte for byte, name for name.

python tools/compare_dumps.py DIR_A DIR_B
Prints every .npy name with `same` or `DIFFERS` (or `only in ...`) and exits 1 on any
difference."""
import os
import sys


def main():
    a, b = sys.argv[1:3]
    names = sorted({f for d in (a, b) for f in os.listdir(d) if f.endswith(".npy")})
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not os.path.exists(pa) or not os.path.exists(pb):
            print(f"{n}: only in {a if os.path.exists(pa) else b}")
            bad += 1
            continue
        with open(pa, "rb") as fa, open(pb, "rb") as fb:
            same = fa.read() == fb.read()
        print(f"{n}: {'same' if same else 'DIFFERS'}")
        bad += not same
    print(f"{len(names)} files, {bad} differing")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main())

"""Host cost of TextChar's wrap serialiser (schema.py: `alternatives` is left out of model_dump while None): model_dump of a page of
characters with the serialiser against a TextChar-shaped model without it.

    python tools/hostbench/dump_cost.py [n_chars]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(n):
    from surya_amd.recognition.schema import BaseChar, TextChar

    class PlainChar(BaseChar):          # TextChar before the field existed
        bbox_valid: bool = True

    poly = [[0, 0], [8, 0], [8, 10], [0, 10]]
    for cls in (PlainChar, TextChar):
        chars = [cls(text="a", polygon=poly, confidence=0.5) for _ in range(n)]
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for c in chars:
                c.model_dump()
            best = min(best, time.perf_counter() - t0)
        print(f"{cls.__name__:10s} model_dump: {best / n * 1e6:.2f} us per character, {best * 1e3:.1f} ms per {n} characters")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10000)

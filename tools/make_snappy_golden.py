"""Writes tests/golden/snappy/: both golden texts as raw Snappy blocks, made by libsnappy's RawCompress through
pyarrow.compress(data, codec="snappy").  The fixtures are committed; this only says how they were made.  pyarrow 25.0.0 wrote the
committed ones."""
import os

import pyarrow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out_dir = os.path.join(ROOT, "tests", "golden", "snappy")
    os.makedirs(out_dir, exist_ok=True)
    for name in ("10x10y", "alice29.txt"):
        with open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
            data = f.read()
        block = pyarrow.compress(data, codec="snappy", asbytes=True)
        assert pyarrow.decompress(block, len(data), codec="snappy", asbytes=True) == data
        with open(os.path.join(out_dir, name + ".block"), "wb") as f:
            f.write(block)
        print(name, len(data), "->", len(block))


if __name__ == "__main__":
    main()

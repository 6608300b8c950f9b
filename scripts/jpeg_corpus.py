"""Write the generated JPEG corpus of the tests (tests/_jpeg_ref.py: the device test's case matrix and the unsupported files) into
a directory - the input of scripts/jpeg_host_check.cpp.

    python scripts/jpeg_corpus.py DIR
"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (os.path.join(ROOT, "salient-object-detection_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main(out):
    import _jpeg_ref as R
    os.makedirs(out, exist_ok=True)
    files = dict(R.case_matrix())
    files.update({"unsupported-" + k: v for k, v in R.unsupported_files().items()})
    for name, data in files.items():
        with open(os.path.join(out, name + ".bin"), "wb") as f:
            f.write(data)
    print(f"{len(files)} files -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])

"""Fixture generator of the structure-search tests (tests/test_structure_search_host.py): the three test complexes of the reference,
``tests/data/inference_data/structures/cifs/{1fyt,5ksa,7t2d}-assembly1.cif``, cut down to what ``StructureSet.from_directory`` reads.

    python tests/golden/make_goldens_search.py      # -> tests/golden/search_structures/<name>-assembly1.cif.gz

Of each file the ``_atom_site`` loop is kept with its column list, and of its rows the CA atoms and every HETATM record (waters and
ligands: rows the feature builder counts and that hold no CA).  Everything else - the other categories, the side chains - is dropped,
which takes a file from 0.7 - 1.4 MB to about a tenth; the text is kept gzip-compressed (no file name or time in the header, so a
rerun writes the same bytes) and the test unpacks it.  Data only: no program text of the reference is copied."""
import gzip
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import refharness as rh  # noqa: E402

CIFS = rh.REF + "/tests/data/inference_data/structures/cifs/{}-assembly1.cif"
NAMES = ("1fyt", "5ksa", "7t2d")
LIMIT = 1 << 20  # the repository's size limit of a committed file


def cut(text: str) -> str:
    lines = text.split("\n")
    first = next(i for i, s in enumerate(lines) if s.startswith("_atom_site."))
    columns = []
    i = first
    while lines[i].startswith("_atom_site."):
        columns.append(lines[i].split(".", 1)[1].strip())
        i += 1
    atom, group = columns.index("label_atom_id"), columns.index("group_PDB")
    kept = []
    while i < len(lines) and lines[i].strip() and not lines[i].startswith("#"):
        t = lines[i].split()
        if t[group] == "HETATM" or t[atom].strip('"') == "CA":
            kept.append(lines[i])
        i += 1
    return "\n".join([lines[0], "#", "loop_"] + lines[first:first + len(columns)] + kept + ["#", ""])


def main():
    out_dir = os.path.join(HERE, "search_structures")
    os.makedirs(out_dir, exist_ok=True)
    for name in NAMES:
        with open(CIFS.format(name)) as f:
            text = cut(f.read())
        assert len(text) < LIMIT
        path = os.path.join(out_dir, f"{name}-assembly1.cif.gz")
        with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.encode())
        print(f"wrote {path} ({len(text)} bytes of text, {os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

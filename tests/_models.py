"""The reference's .vox model assets as stored test inputs under tests/golden/: navigate.vox as it is, the gingerbread
house (3.2 MB) xz-compressed. Test infrastructure."""
import lzma
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = ("navigate.vox", "gingerbread_house_by_kirra_luan.vox")


def model_bytes(name):
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return open(path, "rb").read()
    return lzma.open(path + ".xz").read()


def unpack_model(name, directory):
    """Writes the model into `directory` under its own name (for importers that take a file name); returns the path."""
    path = os.path.join(str(directory), name)
    with open(path, "wb") as f:
        f.write(model_bytes(name))
    return path

"""Names and pictures of image pairs (facenet/utils.py:14-54): what ``FalseExamples.write_false_pairs`` writes."""
from __future__ import annotations

import os

import numpy as np


def _folder_and_stem(file):
    file = str(file)
    return os.path.basename(os.path.dirname(file)), os.path.splitext(os.path.basename(file))[0]


def file2text(file) -> str:
    """'<folder>/<name without extension>' of an image file."""
    return os.path.join(*_folder_and_stem(file))


def generate_filename(dirname, value, file1, file2) -> str:
    """The PNG of a pair inside ``dirname``: 'dir|name1 & name2 & value.png' for two files of one folder,
    'dir1|name1 & dir2|name2 & value.png' otherwise; the value with three decimals."""
    (dir1, name1), (dir2, name2) = _folder_and_stem(file1), _folder_and_stem(file2)
    second = name2 if dir1 == dir2 else '{}|{}'.format(dir2, name2)
    return os.path.join(str(dirname), '{}|{} & {} & {:2.3f}.png'.format(dir1, name1, second, value))


def _font(size):
    from PIL import ImageFont
    try:
        return ImageFont.truetype("LiberationSans-Regular.ttf", size)
    except OSError:           # the font is not installed
        return ImageFont.load_default()


class ConcatenateImages:
    """Two images of equal height side by side, with '<file2text 1> & <file2text 2>' and the distance written in green into the
    top left corner.  ``save(outdir)`` writes it under ``generate_filename``'s name."""

    def __init__(self, file1, file2, distance, font_size=13):
        from PIL import Image, ImageDraw
        self.file1, self.file2, self.distance = file1, file2, distance
        halves = [np.array(Image.open(str(f)).convert("RGB")) for f in (file1, file2)]
        self.img = Image.fromarray(np.concatenate(halves, axis=1))
        text = '{} & {}\n{:2.3f}'.format(file2text(file1), file2text(file2), distance)
        ImageDraw.Draw(self.img).text((0, 0), text, (0, 255, 0), font=_font(font_size))

    def save(self, outdir):
        self.img.save(generate_filename(outdir, self.distance, self.file1, self.file2))

"""BADJA keypoint annotations (Biggs et al., "Creatures great and SMAL"; reference loader: third_party/ext_utils/badja_data.py).

    <root>/joint_annotations/<seqname>.json   a list of {image_path, segmentation_path, joints [37][2] (row, col), visibility [37]}
    <root>/<image_path>, <root>/<segmentation_path>

BADJAData(seqname, root).get_loader() yields (rgb uint8 [H,W,3], sil uint8 [H,W,3], joints int64 [20,2], visible bool [20], name)
per annotated frame whose image and mask both exist, in the file's order; joints and visibility are those of the 20 SMAL joints
BADJA annotates (ANNOTATED_JOINTS).  Images are read with PIL; a palette or grey-scale mask comes back as RGB, so that
sil[..., 0] > 0 is the silhouette as the reference reads it.

Departure: the reference resizes the mask to the image with cv2.resize(sil, (w, h), cv2.INTER_NEAREST), which passes the flag
as the `dst` argument and so resizes bilinearly.  BADJA's masks have their image's size, where that resize is an identity; a
mask of another size raises ValueError here instead of being interpolated.
"""
import json
import os

import numpy as np

# The SMAL joints BADJA annotates, in SMAL order: legs (upper right, upper left, lower right, lower left, three each), neck,
# tail (three), head (two), ears (two).  Exactly the joints ever marked visible in the bear, camel and dog annotations.
ANNOTATED_JOINTS = np.array([8, 9, 10, 12, 13, 14, 15, 18, 19, 20, 22, 23, 24, 25, 28, 31, 32, 33, 35, 36])


def frame_number(name):
    """Frame number of an image path: .../00012.jpg -> 12 (eval_badja.py:171)."""
    return int(os.path.basename(name).split('.')[-2])


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


class BADJAData(object):
    def __init__(self, seqname, root='./database'):
        self.root = root
        path = os.path.join(root, 'joint_annotations', '%s.json' % seqname)
        if not os.path.exists(path):
            raise FileNotFoundError('BADJA annotations not found: %s' % path)
        with open(path) as fh:
            annos = json.load(fh)
        self.entries = []
        for a in annos:
            img = os.path.join(root, a['image_path'])
            seg = os.path.join(root, a['segmentation_path'])
            if os.path.exists(img) and os.path.exists(seg):
                self.entries.append((img, seg, np.asarray(a['joints'], np.int64), np.asarray(a['visibility'], bool)))
            elif os.path.exists(img):
                print('BADJA SEGMENTATION file path: %s is missing' % seg)
            else:
                print('BADJA IMAGE file path: %s is missing' % img)
        print('Loaded BADJA dataset')

    def __len__(self):
        return len(self.entries)

    def get_loader(self):
        for img, seg, joints, visible in self.entries:
            rgb = _read_rgb(img)
            sil = _read_rgb(seg)
            if sil.shape[:2] != rgb.shape[:2]:
                raise ValueError('%s: mask is %dx%d but its image %s is %dx%d (masks are expected at the image size)'
                                 % (seg, sil.shape[0], sil.shape[1], img, rgb.shape[0], rgb.shape[1]))
            yield rgb, sil, joints[ANNOTATED_JOINTS].copy(), visible[ANNOTATED_JOINTS].copy(), img

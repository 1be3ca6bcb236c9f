"""A directory of `<index>_optical.png` / `<index>_thermal.png` pairs as a dataset: what prepare_images.py writes
(`preprocessed/`) and what align_images.py writes (`aligned/best/`), read without building a store first.  The optical file is
8-bit colour or grey, the thermal file 16 bit (an 8-bit one is put on the 16-bit scale); both become fp32 in [0, 1] through
mp_frames_to_float (csrc/pyramid.hip) -- colour / 255 then COLOR_BGR2GRAY, v / 65535 -- and the sample dict is
ImagePairDataset's (build_sample), with its random crop and its draws from `random` in the same order."""
import copy
import os
import random

import numpy as np
from torch.utils.data.dataset import Dataset

from ..utils.utils import dict_update
from .image_pair_dataset import build_sample, check_augmentation_config


def read_png_pair(directory, index):
    """(optical uint8 (H, W) or BGR (H, W, 3), thermal uint16 (H, W)) of pair `index`"""
    from PIL import Image
    with Image.open(os.path.join(directory, index + '_optical.png')) as im:
        if im.mode in ('L', 'P', '1'):
            optical = np.array(im.convert('L'), np.uint8)
        else:
            optical = np.ascontiguousarray(np.array(im.convert('RGB'), np.uint8)[:, :, ::-1])       # BGR, as cv2.imread
    path = os.path.join(directory, index + '_thermal.png')
    with Image.open(path) as im:
        thermal = np.array(im)
    if thermal.ndim != 2:
        raise ValueError('%s: the thermal image must have one channel' % path)
    if thermal.dtype == np.uint8:
        thermal = thermal.astype(np.uint16) * 257           # 8-bit files on the 16-bit scale: v / 255 == 257 v / 65535
    elif thermal.dtype != np.uint16:
        thermal = np.clip(thermal, 0, 65535).astype(np.uint16)
    return optical, thermal


class ImageFilePairs(Dataset):
    default_config = {
        'directory': None,
        'height': -1,
        'width': -1,
        'single_image': True,
        'random_pairs': False,
        'return_name': True,
        'augmentation': {
            'photometric': {'enable': False, 'primitives': 'all', 'params': {}, 'random_order': True},
            'homographic': {'enable': False, 'params': {}, 'border_reflect': True,
                            'valid_border_margin': 0, 'mask_border': True},
        }
    }

    def __init__(self, config):
        self.config = dict_update(copy.deepcopy(self.default_config), config or {})
        directory = self.config['directory']
        if directory is None:
            raise ValueError('ImageFilePairs: The directory of the image pairs needs to be present in the config file')
        check_augmentation_config(self.config, 'ImageFilePairs')
        suffix = '_optical.png'
        indices = [f[:-len(suffix)] for f in os.listdir(directory) if f.endswith(suffix)]
        missing = [i for i in indices if not os.path.isfile(os.path.join(directory, i + '_thermal.png'))]
        if missing:
            raise IndexError('Thermal images for the following samples not available: {}'.format(sorted(missing)))
        self.memberslist = sorted(indices, key=lambda i: (0, int(i), i) if i.isdigit() else (1, 0, i))
        self.num_files = len(self.memberslist)
        print('The directory ' + str(directory) + ' contains {} image pairs'.format(self.num_files))

    def __getitem__(self, index):
        from ..utils import alignment
        name = self.memberslist[index]
        optical, thermal = read_png_pair(self.config['directory'], name)
        if thermal.shape != optical.shape[:2]:
            raise ValueError('ImageFilePairs: The optical and thermal image must have the same shape')
        optical = alignment.frames_to_float(optical, single_bgr=optical.ndim == 3).cpu().numpy()
        thermal = alignment.frames_to_float(thermal).cpu().numpy()
        if self.config['height'] > 0 or self.config['width'] > 0:
            h = self.config['height'] if self.config['height'] > 0 else thermal.shape[0]
            w = self.config['width'] if self.config['width'] > 0 else thermal.shape[1]
            if w > thermal.shape[1] or h > thermal.shape[0]:
                raise ValueError('ImageFilePairs: Requested height/width exceeds original image size')
            i_h = random.randint(0, thermal.shape[0] - h)
            i_w = random.randint(0, thermal.shape[1] - w)
            optical = optical[i_h:i_h + h, i_w:i_w + w]
            thermal = thermal[i_h:i_h + h, i_w:i_w + w]
        return build_sample(optical, thermal, None, self.config, name)

    def get_name(self, index):
        return self.memberslist[index]

    def returns_pair(self):
        return not self.config['single_image']

    def __len__(self):
        return self.num_files

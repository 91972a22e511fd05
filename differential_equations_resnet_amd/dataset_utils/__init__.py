"""Input pipeline (reference: dataset_utils/)."""
from .array_dataset import ArrayDataset, create_tf_dataset_from_arrays
from .cifar10_utils import build_cifar10_dataset, one_hot
from .tf_dataset_preprocessors_image_classification import (ConvertLabelsToOneHot, DecodeImages, DecodeJPEGImages,
                                                            RandomBrightness, RandomCrop, RandomFlipLeftRight,
                                                            RandomSaturation, Resize, ResizeWithPad,
                                                            UnpackImagesLabels, compile_preprocessors)

__all__ = ["ArrayDataset", "create_tf_dataset_from_arrays", "build_cifar10_dataset", "one_hot",
           "UnpackImagesLabels", "ConvertLabelsToOneHot", "DecodeImages", "DecodeJPEGImages", "RandomCrop", "Resize",
           "ResizeWithPad", "RandomFlipLeftRight", "RandomBrightness", "RandomSaturation", "compile_preprocessors"]

"""Host-side mirror of the image compute of the reference's internal/rekognition/rekognition.go: resizeImageIfNeeded (lines 173-259),
which the label service runs on every uploaded image before it asks for labels.  (DetectLabels itself is a cloud call and stays out
of scope.)  An image of at most MaxImageSize bytes is returned as it is; a larger one is decoded, resized into a 2048-pixel box and
written as a JPEG at quality 95 -- the bytes gocv.IMRead / Resize / IMWrite produce, with the reference's own quirk: it reads gocv's
Size() = [rows, cols] as (width, height), so a 4000x3000 landscape photo comes out 1536 wide x 2048 high.
"""
from . import _lib

MaxImageSize = _lib.MAX_IMAGE_SIZE  # 5 * 1024 * 1024
MaxImageDim = _lib.MAX_IMAGE_DIM    # 2048


def resizeImageIfNeeded(imagePath):
    """rekognition.go:173: the file's bytes, downsized if they exceed MaxImageSize (host only, no GPU)."""
    return _lib.downsize_image(imagePath, MaxImageSize, MaxImageDim)


def resizeImageIfNeededBytes(data):
    """resizeImageIfNeeded for an image held in memory (models.UploadedImage.Data)."""
    return _lib.downsize_image_mem(data, MaxImageSize, MaxImageDim)


def resizeImagesIfNeeded(ctx, imagePaths, threads=0):
    """The batched form on a Context: JPEGs above the limit are rebuilt, resized and encoded on the GPU -> (list of bytes, status);
    entry i equals resizeImageIfNeeded(imagePaths[i]); a failed image has an empty entry and a non-zero status."""
    return ctx.downsize_images(imagePaths, MaxImageSize, MaxImageDim, threads)


def resizeImagesIfNeededBytes(ctx, images, threads=0):
    """resizeImagesIfNeeded for images held in memory."""
    return ctx.downsize_images_mem(images, MaxImageSize, MaxImageDim, threads)

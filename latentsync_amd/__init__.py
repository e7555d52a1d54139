def __getattr__(name):
    # resolved on first use, so `import latentsync_amd` stays free of torch
    if name == "ImageProcessor":
        from .image_processor import ImageProcessor
        return ImageProcessor
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

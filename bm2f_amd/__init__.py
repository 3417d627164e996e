"""bm2f_amd — MI355X-native (gfx950) Mask2Former pixel-decoder + transformer-decoder hot path.

Drop-in for the reference's (wenhe-jia/BM2F) MSDeformAttn op, MSDeformAttnPixelDecoder and
MultiScaleMaskedTransformerDecoder, backed by hand-written HIP kernels in ``bm2f_amd/csrc`` reached
through the C ABI of ``include/bm2f.h``.
"""
from . import _native  # noqa: F401
from .inference import (MaskFormerInference, instance_inference, panoptic_inference,  # noqa: F401
                        semantic_inference)
from .mask_criterion import HungarianMatcher, SetCriterion, VideoHungarianMatcher, VideoSetCriterion  # noqa: F401
from .evaluation import (instance_map_annotations, instances_to_coco_json,  # noqa: F401
                         instances_to_coco_json_video, load_sem_seg_predictions, panoptic_to_coco_detection,
                         sem_seg_to_coco_json)
from .label_rle import label_maps_to_rle, rle_to_label_maps  # noqa: F401
from .coco_eval import (COCOEvalResult, COCOEvaluator, COCOGroundTruth, COCOParams,  # noqa: F401
                        evaluate_coco)
from .mask_iou import (mask_iou, mask_pair_counts, mask_pair_counts_ragged, rle_to_bits,  # noqa: F401
                       rle_to_bits_ragged)
from .mask_boundary import boundary_bits_ragged, boundary_dilation, mask_to_boundary_bits  # noqa: F401
from .label_counts import label_histogram_ragged, label_pair_counts, label_pair_counts_ragged  # noqa: F401
from .label_targets import label_targets_to_masks, panoptic_targets, semantic_targets  # noqa: F401
from .panoptic_eval import (COCOPanopticEvaluator, PanopticGroundTruth, PQStat, evaluate_panoptic,  # noqa: F401
                            id2rgb, pq_from_counts, rgb2id)
from .tta import SemanticSegmentorWithTTA, semantic_inference_tta, tta_view_sizes  # noqa: F401
from .image_views import (DeviceTTAMapper, View, image_views, label_views, lsj_view,  # noqa: F401
                          preprocess_test_images, resize_image, resize_shortest_edge_size)
from .color_aug import ColorAug, draw_color_aug_ssd, draw_video_photometric  # noqa: F401
from .train_mappers import (PanopticTrainMapper, SemanticTrainMapper, semantic_train_view,  # noqa: F401
                            video_clip_views)
from .instance_views import bit_boxes_ragged, instance_views  # noqa: F401
from .instance_mappers import (COCOInstanceLSJMapper, InstanceTrainMapper,  # noqa: F401
                               VideoInstanceTrainMapper, sample_clip_frames, transform_polygons)
from .sem_seg_eval import SemSegEvaluator, evaluate_sem_seg, sem_seg_metrics  # noqa: F401
from .polygon import (ann_to_rle, convert_polygons_to_rle, polygon_crossings, polygons_to_bits,  # noqa: F401
                      polygons_to_bits_ragged, polygons_to_rle)
from .rle import counts_to_string, rle_area, rle_decode, rle_encode, string_to_counts  # noqa: F401
from .swin import D2SwinTransformer, SwinTransformer, window_attention  # noqa: F401
from .video_criterion import (VideoHungarianMatcherProj, VideoHungarianMatcherProjPair,  # noqa: F401
                              VideoSetCriterionProj, VideoSetCriterionProjSpatPair,
                              VideoSetCriterionProjSpatPairTempPair)
from .video_inference import VideoMaskFormerInference, pack_mask_bits, unpack_mask_bits  # noqa: F401
from .video_targets import (feat_resize_pad, prepare_video_targets,  # noqa: F401
                            prepare_video_weaksup_targets)
from .ytvis_eval import (YTVISEvalResult, YTVISEvaluator, YTVISGroundTruth, YTVISParams,  # noqa: F401
                         evaluate_ytvis)
from .msda import MSDeformAttn, MSDeformAttnFunction, ms_deform_attn_backward, ms_deform_attn_forward  # noqa: F401

__version__ = "0.1.0"

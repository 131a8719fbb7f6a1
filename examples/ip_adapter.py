"""IP-Adapter image prompts on the SD 1.5 pipeline: load an adapter, set its scale, pass CLIP image embeddings.

    python examples/ip_adapter.py /path/to/stable-diffusion-v1-5 /path/to/ip-adapter_sd15.safetensors out.pt

``ip_adapter_image_embeds`` is what ``CLIPVisionModelWithProjection(...).image_embeds`` gives for the prompt image -- one tensor
[2][num_images][1024] per adapter, the negative (zeros) first -- computed once, outside the step.  Here it is random, as are the text
embeddings, so the script needs no tokenizer or encoder; put your own in their place.  With a fourth and fifth argument -- a local
CLIP vision directory (config.json, model.safetensors, preprocessor_config.json) and an image file -- the engine's own encoder is attached
and the call takes the image itself: ``ip_adapter_image=``."""
import sys

import torch

import diffusers_amd as da

if __name__ == "__main__":
    model_dir, adapter_file, out_file = sys.argv[1:4]
    pipe = da.StableDiffusionPipeline.from_pretrained(model_dir)
    pipe.load_ip_adapter(adapter_file)                      # a local .safetensors file with image_proj.* / ip_adapter.* keys
    pipe.set_ip_adapter_scale(0.6)                          # part of the captured step's key: a new value re-captures once

    g = torch.Generator("cpu").manual_seed(0)
    text, negative = (torch.randn((1, 77, 768), generator=g).to(torch.bfloat16) for _ in range(2))
    image = torch.randn((1, 1, 1024), generator=g).to(torch.bfloat16)
    embeds = [torch.cat([torch.zeros_like(image), image])]  # [negative, positive] under classifier-free guidance

    first = pipe(prompt_embeds=text, negative_prompt_embeds=negative, ip_adapter_image_embeds=embeds, num_inference_steps=25,
                 generator=g).images
    # another image prompt of the same shape replays the captured step: only the image keys / values are refreshed
    other = [torch.cat([torch.zeros_like(image), torch.randn((1, 1, 1024), generator=g).to(torch.bfloat16)])]
    second = pipe(prompt_embeds=text, negative_prompt_embeds=negative, ip_adapter_image_embeds=other, num_inference_steps=25,
                  generator=g).images
    results = {"first": first.cpu(), "second": second.cpu()}
    if len(sys.argv) > 5:
        from PIL import Image
        pipe.image_encoder = da.CLIPVisionModelWithProjection.from_pretrained(sys.argv[4])
        results["image"] = pipe(prompt_embeds=text, negative_prompt_embeds=negative, ip_adapter_image=Image.open(sys.argv[5]),
                                num_inference_steps=25, generator=g).images.cpu()
    torch.save(results, out_file)

    pipe.unload_ip_adapter()                                # the pipeline as it was: cross-attention takes its usual route again
